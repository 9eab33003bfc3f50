// plan_dump — prints the k-NN launch plan (csrc/gkg_knn_plan.h) of every call listed in a case file, one line per case.
// Stand-alone host program: c++ -std=c++17 -I include -I gkgnet_amd/csrc plan_dump.cpp -o plan_dump && ./plan_dump cases.txt
//
// Case line:  role B G c N M k d dtype flags has_y has_relpos ldx xchunk fused        ('#' starts a comment line)
//   role   cm (gkg_knn_fwd, BG = B G), tm (gkg_knn_fwd_tm), tm16 (gkg_knn_fwd_tm16), fused (gkg_knn_mr_fwd_tm), probe
//          (gkg_knn_mr_fused_supported), prodq / prodk (gkg_affine_knn_prep, as_keys = 0 / 1), planq (knn_query_prep_plan)
//   flags  the GKG_KNN_* word;  fused: the consumer of a producer role is gkg_knn_mr_fwd_tm
// Output: line i is case i.  "E code message", or (a probe) ok / no, or the plan:
//   kd KD S tps cp16 cp16p Nr Mr cpad_ws cpad el <norm pf prep_x prep_y as four digits>
//   W  a 32-bit hash of the workspace offsets xh, yh, sqx, sqy, pv, pi, xp, yp, flags (to keep the recorded file small), total bytes
//   T  ku guard buf waves mrf lds_tile grid_x rp_major rp_group          (not for a producer role: it launches its preparation only)
//   P  pf_kdw pf_buf pf_sb lds_pf margin                                  (when the prefilter runs)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gkg_knn_plan.h"

using namespace gkg;

struct Case { char role[8]; int B, G, c, N, M, k, d, dtype; unsigned flags; int has_y, has_rp, ldx, xchunk, fused; };

static bool parse_case(const char* line, Case* cs) {
  return sscanf(line, "%7s %d %d %d %d %d %d %d %d %u %d %d %d %d %d", cs->role, &cs->B, &cs->G, &cs->c, &cs->N, &cs->M, &cs->k, &cs->d,
                &cs->dtype, &cs->flags, &cs->has_y, &cs->has_rp, &cs->ldx, &cs->xchunk, &cs->fused) == 15;
}

static bool role_is(const Case& cs, const char* r) { return strcmp(cs.role, r) == 0; }
static bool role_known(const Case& cs) {
  static const char* const roles[] = {"cm", "tm", "tm16", "fused", "probe", "prodq", "prodk", "planq"};
  for (const char* r : roles) if (role_is(cs, r)) return true;
  return false;
}

static KnnCall to_call(const Case& cs) {
  KnnCall q{};
  q.BG = cs.B * cs.G; q.G_tm = role_is(cs, "cm") ? 0 : cs.G;
  q.c = cs.c; q.N = cs.N; q.M = cs.M; q.k = cs.k; q.dilation = cs.d; q.dtype = cs.dtype; q.flags = cs.flags;
  q.has_y = cs.has_y != 0; q.has_relpos = cs.has_rp != 0; q.ldx = cs.ldx; q.xchunk = cs.xchunk;
  q.role = role_is(cs, "fused") ? KNN_FUSED : role_is(cs, "probe") ? KNN_FUSED_PROBE : role_is(cs, "prodq") ? KNN_PRODUCE_QUERIES
           : role_is(cs, "prodk") ? KNN_PRODUCE_KEYS : role_is(cs, "planq") ? KNN_QUERY_PREP_PLAN : KNN_GRAPH;
  q.consumer_fused = cs.fused != 0;
  return q;
}

static void print_result(FILE* f, const Case& cs, int rc, const char* msg, const KnnPlan& p) {
  if (role_is(cs, "probe")) { fprintf(f, "%s\n", rc == 0 ? "ok" : "no"); return; }
  if (rc != 0) { fprintf(f, "E %d %s\n", rc, msg ? msg : "-"); return; }
  fprintf(f, "%d %d %d %d %d %d %d %d %d %d %d %d%d%d%d", p.kd, p.KD, p.S, p.tps, p.cp16, p.cp16p, p.Nr, p.Mr, p.cpad_ws, p.cpad, p.el, (int)p.norm,
          (int)p.pf, (int)p.prep_x, (int)p.prep_y);
  const size_t off[9] = {p.off_xh, p.off_yh, p.off_sqx, p.off_sqy, p.off_pv, p.off_pi, p.off_xp, p.off_yp, p.off_flags};
  uint32_t h = 2166136261u;                      // FNV-1a over the nine offsets, low byte first
  for (size_t o : off) for (int b = 0; b < 8; ++b) h = (h ^ (uint32_t)((o >> (8 * b)) & 255)) * 16777619u;
  fprintf(f, " W %08x %zu", h, p.total);
  if (role_is(cs, "prodq") || role_is(cs, "prodk") || role_is(cs, "planq")) { fprintf(f, "\n"); return; }
  fprintf(f, " T %d %d %d %d %d %zu %u %d %d", p.ku, (int)p.guard, p.buf, p.waves, (int)p.mrf, p.lds_tile, p.grid_x, p.rp_major, p.rp_group);
  if (p.pf) fprintf(f, " P %d %d %d %zu %.9g", p.pf_kdw, p.pf_buf, (int)p.pf_sb, p.lds_pf, (double)p.margin);
  fprintf(f, "\n");
}

#ifndef PLAN_DUMP_NO_MAIN
int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: plan_dump cases.txt\n"); return 2; }
  FILE* in = fopen(argv[1], "r");
  if (!in) { perror(argv[1]); return 2; }
  char line[512];
  while (fgets(line, sizeof line, in)) {
    line[strcspn(line, "\r\n")] = 0;
    if (line[0] == 0 || line[0] == '#') continue;
    Case cs;
    if (!parse_case(line, &cs) || !role_known(cs)) { fprintf(stderr, "bad case line: %s\n", line); return 2; }
    KnnPlan p;
    const char* msg = nullptr;
    const int rc = knn_plan(to_call(cs), &p, &msg);
    print_result(stdout, cs, rc, msg, p);
  }
  fclose(in);
  return 0;
}
#endif
