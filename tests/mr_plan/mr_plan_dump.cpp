// mr_plan_dump — prints the max-relative aggregation's launch plan (csrc/gkg_mr_plan.h) of every call listed in a case file, one line
// per case.  Stand-alone host program: c++ -std=c++17 -I include -I gkgnet_amd/csrc mr_plan_dump.cpp -o mr_plan_dump && ./mr_plan_dump cases.txt
//
// Case line:  fam B G c N M k mode arg_kind flags self stats dtype ldx xchunk alias argmax        ('#' starts a comment line)
//   fam    bwd (gkg_mr_bwd_tm; stats = 1: gkg_mr_bwd_tm_bnstats), fwd (gkg_mr_fwd_tm), fwd16 (gkg_mr_fwd_tm16), cmf (gkg_mr_fwd, BG = B G),
//          cmb (gkg_mr_bwd)
//   self   1: self graph (no src / gsrc pointer);  dtype: a cm call's dtype, a fwd call's out_dtype;  ldx xchunk: the fwd call's x view;
//          alias: the fwd call's x and out are one pointer;  argmax: it has an argmax output.  Fields a family does not read are 0.
// Output: line i is case i.  "E code message", or the plan:
//   bwd    form [NT ACC U (streaming forms)] STATS cw grid_x grid_y block lds shmax seed_grid gsrc_bytes work
//   fwd    ldx lds schunk write_x grid KS AK bf16 work
//   cm     fallback CH grid_x grid_y grid_z lds seed_grid gsrc_bytes
#include <stdio.h>
#include <string.h>

#include "gkg_mr_plan.h"

using namespace gkg;

struct Case { char fam[8]; int B, G, c, N, M, k, mode, ak; unsigned flags; int self, stats, dtype, ldx, xchunk, alias, argmax; };

static bool parse_case(const char* line, Case* cs) {
  return sscanf(line, "%7s %d %d %d %d %d %d %d %d %u %d %d %d %d %d %d %d", cs->fam, &cs->B, &cs->G, &cs->c, &cs->N, &cs->M, &cs->k, &cs->mode,
                &cs->ak, &cs->flags, &cs->self, &cs->stats, &cs->dtype, &cs->ldx, &cs->xchunk, &cs->alias, &cs->argmax) == 17;
}

static bool fam_is(const Case& cs, const char* f) { return strcmp(cs.fam, f) == 0; }

static const char* const kFormNames[] = {"stream", "stream-f64", "two-sweep", "det-private", "det-walk", "lds-f32", "global-f32"};

static void print_bwd(FILE* f, const MrBwdTmPlan& p) {
  fprintf(f, "%s", kFormNames[p.form]);
  if (p.form == MR_STREAM || p.form == MR_STREAM_F64) fprintf(f, " %d %d %d", p.NT, p.ACC, p.U);
  fprintf(f, " %d %d %u %u %u %zu %d %u %zu %.0f\n", (int)p.STATS, p.cw, p.grid_x, p.grid_y, p.block, p.lds, p.shmax, p.seed_grid, p.gsrc_bytes, p.work);
}
static void print_fwd(FILE* f, const MrFwdTmPlan& p) {
  fprintf(f, "%d %d %d %d %u %d %d %d %.0f\n", p.ldx, p.lds_, p.schunk, p.write_x, p.grid, p.KS, p.AK, (int)p.out_bf16, p.work);
}
static void print_cm(FILE* f, const MrCmPlan& p) {
  fprintf(f, "%d %d %u %u %u %zu %u %zu\n", (int)p.fallback, p.CH, p.grid_x, p.grid_y, p.grid_z, p.lds, p.seed_grid, p.gsrc_bytes);
}
static void print_error(FILE* f, int rc, const char* msg) { fprintf(f, "E %d %s\n", rc, msg ? msg : "-"); }

#ifndef MR_PLAN_DUMP_NO_MAIN
static bool dump_case(FILE* f, const Case& cs) {
  const char* msg = nullptr;
  int rc;
  if (fam_is(cs, "bwd")) {
    MrBwdTmPlan p;
    rc = mr_bwd_tm_plan(MrBwdTmCall{cs.B, cs.G, cs.c, cs.N, cs.M, cs.k, cs.mode, cs.ak, cs.flags, cs.self != 0, cs.stats != 0}, &p, &msg);
    if (rc == 0) print_bwd(f, p);
  } else if (fam_is(cs, "fwd") || fam_is(cs, "fwd16")) {
    MrFwdTmPlan p;
    rc = mr_fwd_tm_plan(MrFwdTmCall{cs.B, cs.G, cs.c, cs.N, cs.M, cs.k, cs.mode, cs.dtype, cs.ak, cs.ldx, cs.xchunk, cs.self == 0, cs.alias != 0,
                                    cs.argmax != 0, fam_is(cs, "fwd16")}, &p, &msg);
    if (rc == 0) print_fwd(f, p);
  } else if (fam_is(cs, "cmf") || fam_is(cs, "cmb")) {
    MrCmPlan p;
    rc = mr_cm_plan(MrCmCall{fam_is(cs, "cmb"), cs.B * cs.G, cs.c, cs.N, cs.M, cs.k, cs.dtype, cs.self != 0}, &p, &msg);
    if (rc == 0) print_cm(f, p);
  } else {
    return false;
  }
  if (rc != 0) print_error(f, rc, msg);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: mr_plan_dump cases.txt\n"); return 2; }
  FILE* in = fopen(argv[1], "r");
  if (!in) { perror(argv[1]); return 2; }
  char line[512];
  while (fgets(line, sizeof line, in)) {
    line[strcspn(line, "\r\n")] = 0;
    if (line[0] == 0 || line[0] == '#') continue;
    Case cs;
    if (!parse_case(line, &cs) || !dump_case(stdout, cs)) { fprintf(stderr, "bad case line: %s\n", line); return 2; }
  }
  fclose(in);
  return 0;
}
#endif
