// block_trace.cpp — the block driver's call trace, on the host.  csrc/gkg_block.hip only calls other extern "C" entry points of
// the library, so everything it does is the list of those calls and their arguments.  This program compiles the driver with every
// callee replaced by a recorder, fills descriptors with fake (never dereferenced) pointers and prints, per case of a cross product
// over the driver's branches, the return code, the calls and — for the backward — the weight-gradient problems it filled.
// tests/test_block_driver_call_trace_host.py compares the output with tests/block_trace/expected.txt.  Host only: nothing of the
// HIP runtime is called and no GPU is opened.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>

#include "gkg_common.h"

namespace {
void put(const void* p) { std::printf(" %#llx", (unsigned long long)(uintptr_t)p); }
void put(std::nullptr_t) { std::printf(" 0"); }
template <class T, std::enable_if_t<std::is_floating_point<T>::value, int> = 0> void put(T v) { std::printf(" %g", (double)v); }
template <class T, std::enable_if_t<std::is_integral<T>::value && std::is_signed<T>::value, int> = 0> void put(T v) { std::printf(" %lld", (long long)v); }
template <class T, std::enable_if_t<std::is_integral<T>::value && !std::is_signed<T>::value, int> = 0> void put(T v) { std::printf(" %llu", (unsigned long long)v); }

template <class... A> int rec(const char* name, A... a) {
  std::printf("%s", name);
  (put(a), ...);
  std::printf("\n");
  return 0;
}
int g_dgrad_stats_supported = 1;   // what gkg_linear_dgrad_x6_bnbwd_sk_supported answers
int g_scatter_stats_rc = 0;        // what gkg_mr_bwd_tm_bnstats returns
template <class... A> int rec_supported(A... a) { rec("gkg_linear_dgrad_x6_bnbwd_sk_supported", a...); return g_dgrad_stats_supported; }
template <class... A> int rec_scatter(A... a) { rec("gkg_mr_bwd_tm_bnstats", a...); return g_scatter_stats_rc; }
}  // namespace

int gkg_fail(int code, const char* msg) {
  std::printf("gkg_fail %d %s\n", code, msg);
  return code;
}

// one line per callee of the driver
#define gkg_nchw_to_tm(...) rec("gkg_nchw_to_tm", __VA_ARGS__)
#define gkg_nchw_to_tm_add(...) rec("gkg_nchw_to_tm_add", __VA_ARGS__)
#define gkg_nchw_to_tm_add_bnstats(...) rec("gkg_nchw_to_tm_add_bnstats", __VA_ARGS__)
#define gkg_tm_affine_to_nchw(...) rec("gkg_tm_affine_to_nchw", __VA_ARGS__)
#define gkg_tm_affine_to_nchw_dual(...) rec("gkg_tm_affine_to_nchw_dual", __VA_ARGS__)
#define gkg_linear_bn_fwd_x6_sk(...) rec("gkg_linear_bn_fwd_x6_sk", __VA_ARGS__)
#define gkg_bn_apply_train(...) rec("gkg_bn_apply_train", __VA_ARGS__)
#define gkg_bn_apply_train_dual(...) rec("gkg_bn_apply_train_dual", __VA_ARGS__)
#define gkg_bn_apply_knn_prep(...) rec("gkg_bn_apply_knn_prep", __VA_ARGS__)
#define gkg_bn_eval_affine(...) rec("gkg_bn_eval_affine", __VA_ARGS__)
#define gkg_affine_act(...) rec("gkg_affine_act", __VA_ARGS__)
#define gkg_affine_knn_prep(...) rec("gkg_affine_knn_prep", __VA_ARGS__)
#define gkg_knn_mr_fwd_tm(...) rec("gkg_knn_mr_fwd_tm", __VA_ARGS__)
#define gkg_knn_fwd_tm(...) rec("gkg_knn_fwd_tm", __VA_ARGS__)
#define gkg_knn_fwd_tm16(...) rec("gkg_knn_fwd_tm16", __VA_ARGS__)
#define gkg_mr_fwd_tm(...) rec("gkg_mr_fwd_tm", __VA_ARGS__)
#define gkg_mr_fwd_tm16(...) rec("gkg_mr_fwd_tm16", __VA_ARGS__)
#define gkg_mr_bwd_tm(...) rec("gkg_mr_bwd_tm", __VA_ARGS__)
#define gkg_mr_bwd_tm_bnstats(...) rec_scatter(__VA_ARGS__)
#define gkg_bn_bwd_atomic(...) rec("gkg_bn_bwd_atomic", __VA_ARGS__)
#define gkg_bn_bwd_apply_from_sums(...) rec("gkg_bn_bwd_apply_from_sums", __VA_ARGS__)
#define gkg_bn_eval_bwd(...) rec("gkg_bn_eval_bwd", __VA_ARGS__)
#define gkg_linear_dgrad_x6_sk(...) rec("gkg_linear_dgrad_x6_sk", __VA_ARGS__)
#define gkg_linear_dgrad_x6_nchw(...) rec("gkg_linear_dgrad_x6_nchw", __VA_ARGS__)
#define gkg_linear_dgrad_x6_bnbwd_sk(...) rec("gkg_linear_dgrad_x6_bnbwd_sk", __VA_ARGS__)
#define gkg_linear_dgrad_x6_bnbwd_sk_supported(...) rec_supported(__VA_ARGS__)

#include "gkg_block.hip"

namespace {

// a fake pointer that names the field it sits in: 1 MiB x (1 + the field's 8-byte slot in its descriptor)
template <class T> void fake(T*& f, const void* origin) {
  f = reinterpret_cast<T*>((uintptr_t)0x100000u * (uintptr_t)(1 + (reinterpret_cast<const char*>(&f) - static_cast<const char*>(origin)) / 8));
}

enum Want { WANT_NONE, WANT_ALL, WANT_ONE_DBIAS };

void fill_proj(GkgProjBN& p, const void* o, int cin, int cout, int nb, bool frozen, int want, bool the_one) {
  fake(p.planes_fwd, o); fake(p.planes_dgrad, o); fake(p.gamma, o); fake(p.beta, o); fake(p.bias, o);
  fake(p.running_mean, o); fake(p.running_var, o); fake(p.nbt, o);
  p.momentum = 0.1f; p.eps = 1e-5f;
  p.cin = cin; p.cout = cout; p.nb = nb;
  fake(p.fsum, o); fake(p.fzero, o); p.fzero_n = (size_t)2 * nb * cout;
  fake(p.bsum, o); fake(p.bzero, o); p.bzero_n = (size_t)2 * nb * cout + 1;
  fake(p.Y, o); fake(p.bn, o); fake(p.dw, o);
  if (!frozen || want == WANT_ALL) { fake(p.dgamma, o); fake(p.dbeta, o); }
  if (frozen && (want == WANT_ALL || (want == WANT_ONE_DBIAS && the_one))) fake(p.dbias, o);
}

// form 0: fused_mr; 1: two launches, u16 lists; 2: two launches, int64 lists; 3: fused_mr returning the int64 lists
void fill_graph(GkgGraphOp& g, const void* o, bool prep, int form, bool relpos) {
  g.G = 2; g.k = 3; g.d = 1;
  g.fused_mr = form == 0 || form == 3;
  if (relpos) fake(g.relpos, o);
  g.knn_flags = GKG_KNN_NORMALIZE | GKG_KNN_RELPOS_UNIT | GKG_KNN_Y_PREPARED | (prep ? GKG_KNN_X_PREPARED : 0u);
  g.mr_flags = 5u;
  fake(g.knn_ws, o); g.knn_ws_bytes = 4096;
  fake(g.arg, o);
  if (form == 1) fake(g.nn16, o);
  if (form >= 2) { fake(g.nn_idx, o); fake(g.center, o); }
}

constexpr int kB = 2, kC = 64, kH = 3, kW = 3, kL = 5, kM = 9, kCf = 128;

GkgGrapherBlock grapher(bool frozen, int want) {
  GkgGrapherBlock b;
  std::memset(&b, 0, sizeof b);
  const void* o = &b;
  b.B = kB; b.C = kC; b.H = kH; b.W = kW;
  fake(b.x, o); fake(b.out, o); fake(b.xt, o); fake(b.XM, o); fake(b.A2, o);
  fill_proj(b.fc1, o, kC, kC, 1, frozen, want, false);
  fill_proj(b.conv, o, kC / 2, kC / 2, 4, frozen, want, true);
  fill_proj(b.fc2, o, 2 * kC, kC, 1, frozen, want, false);
  fake(b.dout, o); fake(b.dx, o); fake(b.g3, o); fake(b.dY3, o); fake(b.dA2, o); fake(b.dY2, o); fake(b.dXM, o); fake(b.gx1, o);
  fake(b.dY1, o); fake(b.dxt, o);
  b.bn_frozen = frozen;
  return b;
}

GkgLabelBlock label(bool frozen, int want) {
  GkgLabelBlock b;
  std::memset(&b, 0, sizeof b);
  const void* o = &b;
  b.B = kB; b.C = kC; b.L = kL; b.M = kM;
  fake(b.e, o); fake(b.ft, o); fake(b.out, o); fake(b.XM, o); fake(b.A2, o); fake(b.h2, o); fake(b.f1, o);
  fill_proj(b.fc1, o, kC, kC, 1, frozen, want, false);
  fill_proj(b.conv, o, kC / 2, kC / 2, 4, frozen, want, false);
  fill_proj(b.fc2, o, 2 * kC, kC, 1, frozen, want, false);
  fill_proj(b.ffn1, o, kC, kCf, 1, frozen, want, true);
  fill_proj(b.ffn2, o, kCf, kC, 1, frozen, want, false);
  fake(b.dout, o); fake(b.de, o); fake(b.dft, o); fake(b.dY5, o); fake(b.df1, o); fake(b.dY4, o); fake(b.dh2, o); fake(b.dY3, o);
  fake(b.dA2, o); fake(b.dY2, o); fake(b.dXM, o); fake(b.gx1, o); fake(b.dY1, o);
  b.bn_frozen = frozen;
  return b;
}

void print_wq(const GkgWgradProblem* wq, int n) {
  for (int i = 0; i < n; ++i) {
    const GkgWgradProblem& q = wq[i];
    std::printf("wq[%d]", i);
    put(q.dy); put(q.x); put(q.dw); put(q.g_bstride); put(q.x_bstride); put(q.ldg); put(q.ldx); put(q.R); put(q.cin); put(q.cout);
    put(q.nb); put(q.kperm);
    std::printf("\n");
  }
}

void forward_cases(bool is_label, bool frozen) {
  void* const st = reinterpret_cast<void*>((uintptr_t)0x57000000u);
  for (int prep = 0; prep < 2; ++prep)
    for (int form = 0; form < 4; ++form)
      for (int relpos = 0; relpos < 2; ++relpos)
        for (int outs = 0; outs < (is_label ? 1 : 3); ++outs) {
          std::printf("== case %s_fwd frozen=%d prep=%d graph=%d relpos=%d outs=%d\n", is_label ? "label" : "grapher", (int)frozen, prep, form,
                      relpos, outs);
          int rc;
          if (is_label) {
            GkgLabelBlock b = label(frozen, WANT_NONE);
            fill_graph(b.graph, &b, prep, form, relpos);
            fake(b.sk_ws, &b); b.sk_bytes = 1 << 20;
            rc = gkg_grapher_label_fwd(&b, st);
          } else {
            GkgGrapherBlock b = grapher(frozen, WANT_NONE);
            fill_graph(b.graph, &b, prep, form, relpos);
            fake(b.sk_ws, &b); b.sk_bytes = 1 << 20;
            if (outs >= 1) fake(b.out_tm, &b);
            if (outs == 2) {
              b.keys_G = 4; b.keys_L = kL; b.keys_k = 2; b.keys_d = 1; b.keys_fused_mr = 1; b.keys_flags = GKG_KNN_NORMALIZE;
              fake(b.keys_ws, &b); b.keys_ws_bytes = 8192;
            }
            rc = gkg_grapher_fwd(&b, st);
          }
          std::printf("rc %d\n", rc);
        }
}

void backward_cases(bool is_label, bool frozen) {
  void* const st = reinterpret_cast<void*>((uintptr_t)0x57000000u);
  for (unsigned flags = 0; flags < 4; ++flags)
    for (int supported = 0; supported < 2; ++supported)
      for (int scatter = 0; scatter < 2; ++scatter)
        for (int sk = 0; sk < 2; ++sk)
          for (int dtm = 0; dtm < (is_label ? 1 : 2); ++dtm)
            for (int want = 0; want < (frozen ? 3 : 1); ++want) {
              std::printf("== case %s_bwd frozen=%d flags=%u supported=%d scatter_stats=%d sk_ws=%d dout_tm=%d want=%d\n",
                          is_label ? "label" : "grapher", (int)frozen, flags, supported, scatter, sk, dtm, want);
              g_dgrad_stats_supported = supported;
              g_scatter_stats_rc = scatter ? 0 : GKG_ERR_UNSUPPORTED;
              GkgWgradProblem wq[5];
              std::memset(wq, 0, sizeof wq);
              int rc;
              if (is_label) {
                GkgLabelBlock b = label(frozen, want);
                fill_graph(b.graph, &b, true, 3, false);
                if (sk) { fake(b.sk_ws, &b); b.sk_bytes = 1 << 20; }
                b.bwd_flags = flags;
                rc = gkg_grapher_label_bwd(&b, wq, st);
              } else {
                GkgGrapherBlock b = grapher(frozen, want);
                fill_graph(b.graph, &b, true, 0, true);
                if (sk) { fake(b.sk_ws, &b); b.sk_bytes = 1 << 20; }
                if (dtm) fake(b.dout_tm, &b);
                b.bwd_flags = flags;
                rc = gkg_grapher_bwd(&b, wq, st);
              }
              std::printf("rc %d\n", rc);
              print_wq(wq, is_label ? 5 : 3);
            }
}

}  // namespace

int main() {
  for (int is_label = 0; is_label < 2; ++is_label)
    for (int frozen = 0; frozen < 2; ++frozen) {
      forward_cases(is_label, frozen);
      backward_cases(is_label, frozen);
    }
  return 0;
}
