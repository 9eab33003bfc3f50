// bf16-contraction instantiations of the k-NN tile kernel (GKG_KNN_BF16_CONTRACT: the bf16-autocast inference form) —
// their own translation unit so that they compile beside the fp32 forms of gkg_knn.hip.
// The same source with GKG_KNN_EL_PART defined to KNN_EL_F16 gives the fp16-contraction instantiations (GKG_KNN_F16_CONTRACT:
// gkg_knn_hf.hip / gkg_knn_hf_norp.hip): one selection rule for both 16-bit formats.
#include "gkg_knn_tile.h"

using namespace gkg;

#ifndef GKG_KNN_EL_PART
#define GKG_KNN_EL_PART KNN_EL_BF16
#define GKG_KNN_EL_LAUNCHER launch_knn_tile_bf
#endif

// 16-bit matrix-core contraction (GKG_KNN_BF16_CONTRACT / GKG_KNN_F16_CONTRACT), KU 4.  The forms this unit holds, by the plan's
// fields: direct selection with the guard (every list size); lists up to 36: buffered with 12 entries per lane, with KNN_BUF (lists
// above 12), and one wave per 64-query tile (see the kernel's NWV) with 12 (9-entry list) or KNN_BUF entries.  Why each: knn_plan.
// (The forms without a bias: gkg_knn_bf_norp.hip, the same source with GKG_KNN_NORP_PART defined.)
template <int KD, bool HAS_RP>
static hipError_t launch_tile_bf(const KnnArgs& a, const KnnPlan& p, hipStream_t st) {
  constexpr int EL = GKG_KNN_EL_PART;
  GkgProfScope prof(GKG_PROF_KNN_TILE, st);
  if (p.el != EL || p.ku != 4 || p.mrf) return hipErrorInvalidValue;
  if constexpr (KD <= 36) {
    constexpr int SBUF = KD <= 12 ? 12 : KNN_BUF;
    if (!p.guard && p.waves == 1 && p.buf == SBUF) return launch_tile_v<KD, HAS_RP, 4, false, SBUF, EL, 1>(a, p, st);
    if (!p.guard && p.waves == NW && p.buf == 12) return launch_tile_v<KD, HAS_RP, 4, false, 12, EL>(a, p, st);
    if constexpr (KD > 12) {
      if (!p.guard && p.waves == NW && p.buf == KNN_BUF) return launch_tile_v<KD, HAS_RP, 4, false, KNN_BUF, EL>(a, p, st);
    }
  }
  if (p.guard && p.waves == NW && p.buf == 0) return launch_tile_v<KD, HAS_RP, 4, true, 0, EL>(a, p, st);
  return hipErrorInvalidValue;
}

GKG_KNN_LAUNCHER(GKG_KNN_EL_LAUNCHER, launch_tile_bf, 64)
