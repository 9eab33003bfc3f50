// fp16-contraction instantiations of the k-NN tile kernel (GKG_KNN_F16_CONTRACT) with a positional bias: the source of
// gkg_knn_bf.hip — same selection rules — with the element format set to fp16, compiled beside it.
#define GKG_KNN_EL_PART KNN_EL_F16
#define GKG_KNN_EL_LAUNCHER launch_knn_tile_hf
#include "gkg_knn_bf.hip"
