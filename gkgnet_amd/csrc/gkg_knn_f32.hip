// fp32-contract instantiations of the k-NN tile kernel (direct / guard-less / buffered selection) — their own translation
// unit, compiled twice: with the positional bias here, without it in gkg_knn_f32_norp.hip (GKG_KNN_NORP_PART).
#include "gkg_knn_tile.h"

using namespace gkg;

// GKG_KNN_MR_PART (gkg_knn_f32_mr.hip / gkg_knn_f32_mr_norp.hip): the same forms with the max-relative aggregation in the
// epilogue (knn_tile_kernel<..., MRF = true>), modes 0-2.
#ifdef GKG_KNN_MR_PART
constexpr bool kMRF = true;
#define GKG_KNN_F32_LAUNCHER launch_knn_tile_f32_mr
#else
constexpr bool kMRF = false;
#define GKG_KNN_F32_LAUNCHER launch_knn_tile_f32
#endif

// The forms this unit holds, by the plan's fields: direct selection with the ballot guard (KU 4 / 8, every list size), without it
// (9-entry list), buffered selection (KNN_BUF entries, lists up to 36; KU 4 / 8, and 6 without aggregation) and — without
// aggregation — the buffered forms with ONE wave per workgroup.  Why each is chosen: knn_plan.
template <int KD, bool HAS_RP>
static hipError_t launch_tile_f32(const KnnArgs& a, const KnnPlan& p, hipStream_t st) {
  if (p.el != KNN_EL_F32 || p.mrf != kMRF) return hipErrorInvalidValue;
  GkgProfScope prof(GKG_PROF_KNN_TILE, st);
  const bool direct = p.buf == 0 && p.waves == NW, buffered = p.buf == KNN_BUF && !p.guard;
  if constexpr (KD <= 36) {
    if constexpr (!kMRF) {
      if (buffered && p.waves == 1) {
        if (p.ku == 6) return launch_tile_v<KD, HAS_RP, 6, false, KNN_BUF, false, 1>(a, p, st);
        if (p.ku == 8) return launch_tile_v<KD, HAS_RP, 8, false, KNN_BUF, false, 1>(a, p, st);
        if (p.ku == 4) return launch_tile_v<KD, HAS_RP, 4, false, KNN_BUF, false, 1>(a, p, st);
      }
      if (buffered && p.waves == NW && p.ku == 6) return launch_tile_v<KD, HAS_RP, 6, false, KNN_BUF, false, NW, false>(a, p, st);
    }
    if (buffered && p.waves == NW && p.ku == 8) return launch_tile_v<KD, HAS_RP, 8, false, KNN_BUF, false, NW, kMRF>(a, p, st);
    if (buffered && p.waves == NW && p.ku == 4) return launch_tile_v<KD, HAS_RP, 4, false, KNN_BUF, false, NW, kMRF>(a, p, st);
  }
  if constexpr (KD == 9) {
    if (direct && !p.guard && p.ku == 8) return launch_tile_v<KD, HAS_RP, 8, false, 0, false, NW, kMRF>(a, p, st);
    if (direct && !p.guard && p.ku == 4) return launch_tile_v<KD, HAS_RP, 4, false, 0, false, NW, kMRF>(a, p, st);
  }
  if (direct && p.guard && p.ku == 8) return launch_tile_v<KD, HAS_RP, 8, true, 0, false, NW, kMRF>(a, p, st);
  if (direct && p.guard && p.ku == 4) return launch_tile_v<KD, HAS_RP, 4, true, 0, false, NW, kMRF>(a, p, st);
  return hipErrorInvalidValue;
}

GKG_KNN_LAUNCHER(GKG_KNN_F32_LAUNCHER, launch_tile_f32, (kMRF ? 36 : 64))          // the fused forms stop at 36-entry lists
