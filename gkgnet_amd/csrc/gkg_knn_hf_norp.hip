// The fp16-contraction k-NN tile kernel without a positional bias: gkg_knn_hf.hip's settings on the source of
// gkg_knn_bf_norp.hip, compiled beside them.
#define GKG_KNN_NORP_PART 1
#define GKG_KNN_EL_PART KNN_EL_F16
#define GKG_KNN_EL_LAUNCHER launch_knn_tile_hf
#include "gkg_knn_bf.hip"
