// x6_plan_dump — prints the launch plan (csrc/gkg_x6_plan.h) of every split-bf16 GEMM / weight-gradient call listed in a case file, one
// line per case.  Stand-alone host program: c++ -std=c++17 -I include -I gkgnet_amd/csrc x6_plan_dump.cpp -o x6_plan_dump && ./x6_plan_dump cases.txt
//
// Case lines ('#' starts a comment line):
//   g role R cin cout nb ws flags res train slots lda abs ldc cbs aal n1 n2 n3
//       role   fwd (gkg_linear_bn_fwd_x6_sk), dgrad (gkg_linear_dgrad_x6_sk), nchw (gkg_linear_dgrad_x6_nchw), bnbwd (gkg_linear_dgrad_x6_bnbwd_sk)
//       ws     split-K workspace: 0 none, 1 gkg_x6_splitk_workspace_bytes(), 2 16 bytes short, 3 misaligned
//       res    a residual;  slots: resident workgroups of the device (the walk form's input)
//       lda abs   the activation operand's pitch / batch stride (0: contiguous);  ldc cbs: dgrad's dx pitch / batch stride (0: contiguous)
//       aal    the activation operand is 16-byte aligned;  n1 n2 n3: nchw B, N, dx aligned; bnbwd pnb, pco, pact; else 0
//   w mode val R cin cout nb ldg ldx gbs xbs al kperm       mode alone (gkg_linear_wgrad_x6) or det (gkg_linear_wgrad_x6_det, val = slabs)
//   wb det ups n P...        gkg_linear_wgrad_x6_batch (det 0) / _batch_det (1), P = R,cin,cout,nb,ldg,ldx,al,kperm (contiguous batches; al 2: dy is NULL; a list shorter than n repeats)
//   q slabs R cin cout nb ldg ldx al ups slabs      gkg_linear_wgrad_x6_det_slabs
//   q wsb R cin cout nb ldg ldx slabs               gkg_linear_wgrad_x6_det_workspace_bytes
//   q sup R cin res ws flags                        gkg_linear_dgrad_x6_bnbwd_sk_supported
// Output: line i is case i.  "E code message", or
//   g    [2L] body epi NI BN mtiles ntiles ksplit kper grid_x grid_y lds NP KC p_bstride nslots work      (2L: the nchw call's two-launch form)
//   w    wide swap kperm M rows M N mtiles ntiles splits rows_per_split share ubase urem grid_x R rows row0 splits rows_per_split grid_x
//   wb   per launch, in launch order: "B n workgroups [i wide rot end <M fields>]..." or "R i <R fields>"; det: "F workspace-bytes" last
//   q    slabs: n and a checksum of (first_row, rows);  wsb: bytes;  sup: 0 / 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "gkg_x6_plan.h"

using namespace gkg;

static const char* const kBody[] = {"ks", "tile", "walk"};

static void print_error(FILE* f, int rc, const char* msg) { fprintf(f, "E %d %s\n", rc, msg ? msg : "-"); }

static void print_gemm(FILE* f, const X6GemmPlan& p) {
  fprintf(f, "%s%s %d %d %d %d %d %d %d %u %u %zu %d %d %zu %d %.0f\n", p.two_launch ? "2L " : "", kBody[p.body], p.epi, p.NI, p.BN, p.mtiles,
          p.ntiles, p.ksplit, p.kper, p.grid_x, p.grid_y, p.lds, p.NP, p.KC, p.p_bstride, p.nslots, p.work);
}
static void print_main(FILE* f, const X6WgradPart& m) {
  fprintf(f, "M %d %d %d %d %d %d %d %d %d %d %d", m.rows, m.M, m.N, m.mtiles, m.ntiles, m.splits, m.rows_per_split, m.share, m.ubase, m.urem, m.grid_x);
}
static void print_rest(FILE* f, const X6WgradPart& t) { fprintf(f, "R %d %d %d %d %d", t.rows, t.row0, t.splits, t.rows_per_split, t.grid_x); }
static const X6WgradPart kNone{};
static void print_wgrad(FILE* f, const X6WgradPlan& pl) {
  const bool m = pl.main.rows > 0;        // the tile shape shows in the LDS-DMA launch only
  fprintf(f, "%d %d %d ", (int)(m && pl.wide), (int)(m && pl.swap), pl.kperm);
  print_main(f, m ? pl.main : kNone);
  fprintf(f, " ");
  print_rest(f, pl.rest.rows > 0 ? pl.rest : kNone);
  fprintf(f, "\n");
}
static unsigned slab_checksum(unsigned h, int first_row, int rows) { return (h * 31u + (unsigned)first_row) * 31u + (unsigned)rows; }

static bool dump_gemm(FILE* f, char* args) {
  char role[8];
  int R, cin, cout, nb, ws, res, train, slots, lda, ldc, aal, n1, n2, n3;
  unsigned flags;
  size_t abs_, cbs;
  if (sscanf(args, "%7s %d %d %d %d %d %u %d %d %d %d %zu %d %zu %d %d %d %d", role, &R, &cin, &cout, &nb, &ws, &flags, &res, &train, &slots,
             &lda, &abs_, &ldc, &cbs, &aal, &n1, &n2, &n3) != 18)
    return false;
  const bool fwd = strcmp(role, "fwd") == 0;
  X6GemmCall q{};
  q.role = fwd ? X6R_FWD : strcmp(role, "dgrad") == 0 ? X6R_DGRAD : strcmp(role, "nchw") == 0 ? X6R_DGRAD_NCHW : X6R_DGRAD_BNBWD;
  if (q.role == X6R_DGRAD_BNBWD && strcmp(role, "bnbwd") != 0) return false;
  q.M = R; q.N = fwd ? cout : cin; q.K = fwd ? cin : cout; q.nb = nb;
  q.lda = lda ? lda : q.K; q.a_bstride = abs_ ? abs_ : (q.role == X6R_FWD || q.role == X6R_DGRAD ? (size_t)R * q.lda : 0); q.a_aligned = aal != 0;
  q.ldc = ldc; q.c_bstride = cbs;
  q.has_ws = ws != 0; q.ws_aligned = ws != 3; q.ws_bytes = ws == 0 ? 0 : ws == 2 ? X6_SK_BYTES - 16 : X6_SK_BYTES;
  q.flags = flags; q.has_residual = res != 0; q.train = train; q.slots = slots;
  if (q.role == X6R_DGRAD_NCHW) { q.nchw_b = n1; q.nchw_n = n2; q.dx_aligned = n3 != 0; }
  if (q.role == X6R_DGRAD_BNBWD) { q.pnb = n1; q.pco = n2; q.pact = n3; }
  X6GemmPlan p;
  const char* msg = nullptr;
  if (const int rc = x6_gemm_plan(q, &p, &msg)) print_error(f, rc, msg);
  else print_gemm(f, p);
  return true;
}

static bool dump_wgrad(FILE* f, char* args) {
  char mode[8];
  int val, R, cin, cout, nb, ldg, ldx, al, kperm;
  size_t gbs, xbs;
  if (sscanf(args, "%7s %d %d %d %d %d %d %d %zu %zu %d %d", mode, &val, &R, &cin, &cout, &nb, &ldg, &ldx, &gbs, &xbs, &al, &kperm) != 12) return false;
  const bool det = strcmp(mode, "det") == 0;
  if (!det && strcmp(mode, "alone") != 0) return false;
  X6WgradPlan pl;
  const char* msg = nullptr;
  if (det && (val < 0 || val > 4096)) { print_error(f, GKG_ERR_SHAPE, "gkg_linear_wgrad_x6_det: slabs out of range (0 .. 4096)"); return true; }
  int rc = x6_wgrad_plan(X6WgradCall{R, cin, cout, nb, ldg, ldx, gbs, xbs, al != 0, 0, kperm, det ? val : 0}, &pl, &msg);
  if (rc == 0 && det && !x6_wdet_elems_ok(cin, cout, nb)) { rc = GKG_ERR_UNSUPPORTED; msg = "gkg_linear_wgrad_x6_det: more than 2^31 elements of dw"; }
  if (rc) print_error(f, rc, msg);
  else print_wgrad(f, pl);
  return true;
}

static bool dump_batch(FILE* f, char* args) {
  int det, ups, n, used = 0;
  if (sscanf(args, "%d %d %d%n", &det, &ups, &n, &used) != 3 || n < 0 || n > 4096) return false;
  std::vector<GkgWgradProblem> p((size_t)n);
  char* const s0 = args + used;
  char* s = s0;
  for (int i = 0; i < n; ++i) {
    int R, cin, cout, nb, ldg, ldx, al, kperm, adv = 0;
    if (sscanf(s, " %d,%d,%d,%d,%d,%d,%d,%d%n", &R, &cin, &cout, &nb, &ldg, &ldx, &al, &kperm, &adv) != 8) {
      if (s == s0 || *(s + strspn(s, " ")) != 0) return false;
      s = s0;                       // fewer problems listed than n: the list repeats
      if (sscanf(s, " %d,%d,%d,%d,%d,%d,%d,%d%n", &R, &cin, &cout, &nb, &ldg, &ldx, &al, &kperm, &adv) != 8) return false;
    }
    s += adv;
    GkgWgradProblem& q = p[(size_t)i];
    memset(&q, 0, sizeof q);
    // dummy operands: only nullness and alignment are read; dw's distance from the base tells the problems apart
    q.dy = al == 2 ? nullptr : reinterpret_cast<const float*>((size_t)0x10000000 + (al ? 0 : 4)); q.x = reinterpret_cast<const float*>((size_t)0x20000000);
    q.dw = reinterpret_cast<float*>((size_t)0x40000000 + (size_t)i * 0x100000);
    q.R = R; q.cin = cin; q.cout = cout; q.nb = nb; q.ldg = ldg; q.ldx = ldx; q.kperm = kperm;
    q.g_bstride = (size_t)R * ldg; q.x_bstride = (size_t)R * ldx;
  }
  static X6WgradBatchPlan bp;
  const char* msg = nullptr;
  if (const int rc = x6_wgrad_batch_plan(n ? p.data() : nullptr, n, ups, det != 0, &bp, &msg)) { print_error(f, rc, msg); return true; }
  std::string group;                // the open group's problems; it is launched when it is full, the remainders in between
  int open = 0;
  int last_end = 0;
  std::vector<std::string> out;
  char buf[512];
  for (int oi = 0; oi < n; ++oi) {
    const X6WgradPlan& pl = bp.pl[oi];
    if (bp.slot[oi] >= 0) {
      const X6WgradPart& m = pl.main;
      snprintf(buf, sizeof buf, " [%d %d %d %d %d %d M %d %d %d %d %d %d %d %d %d %d %d]", bp.order[oi], (int)pl.wide, (int)pl.swap, pl.kperm, bp.rot[oi],
               bp.end[oi], m.rows, m.M, m.N, m.mtiles, m.ntiles, m.splits, m.rows_per_split, m.share, m.ubase, m.urem, m.grid_x);
      group += buf;
      last_end = bp.end[oi];
      if (++open == X6W_BATCH) {
        out.push_back("B " + std::to_string(open) + " " + std::to_string(last_end) + group);
        group.clear(); open = 0;
      }
    }
    if (pl.rest.rows > 0) {
      const X6WgradPart& t = pl.rest;
      snprintf(buf, sizeof buf, "R %d %d %d %d %d %d", bp.order[oi], t.rows, t.row0, t.splits, t.rows_per_split, t.grid_x);
      out.push_back(buf);
    }
  }
  if (open) out.push_back("B " + std::to_string(open) + " " + std::to_string(last_end) + group);
  if (det) out.push_back("F " + std::to_string((bp.det_floats * 4 + 15) & ~(size_t)15));
  for (size_t i = 0; i < out.size(); ++i) fprintf(f, "%s%s", i ? " ; " : "", out[i].c_str());
  fprintf(f, "\n");
  return true;
}

static bool dump_query(FILE* f, char* args) {
  char what[8];
  int used = 0;
  if (sscanf(args, "%7s%n", what, &used) != 1) return false;
  args += used;
  const char* msg = nullptr;
  if (strcmp(what, "slabs") == 0) {
    int R, cin, cout, nb, ldg, ldx, al, ups, slabs;
    if (sscanf(args, "%d %d %d %d %d %d %d %d %d", &R, &cin, &cout, &nb, &ldg, &ldx, &al, &ups, &slabs) != 9) return false;
    X6WgradPlan pl;
    if (const int rc = x6_wgrad_plan(X6WgradCall{R, cin, cout, nb, ldg, ldx, 0, 0, al != 0, ups, 0, ups > 0 ? 0 : slabs}, &pl, &msg)) {
      print_error(f, rc, msg);
      return true;
    }
    unsigned h = 0;
    for (int s = 0; s < pl.slabs(); ++s) {
      int first = 0, rows = 0;
      pl.slab_rows(s, &first, &rows);
      h = slab_checksum(h, first, rows);
    }
    fprintf(f, "%d %u\n", pl.slabs(), h);
  } else if (strcmp(what, "wsb") == 0) {
    int R, cin, cout, nb, ldg, ldx, slabs, rc = 0;
    if (sscanf(args, "%d %d %d %d %d %d %d", &R, &cin, &cout, &nb, &ldg, &ldx, &slabs) != 7) return false;
    const int S = x6_wdet_elems_ok(cin, cout, nb) ? x6_wdet_max_slabs(R, cin, cout, nb, ldg, ldx, slabs, &rc, &msg) : 0;
    fprintf(f, "%zu\n", ((size_t)S * nb * cout * cin * 4 + 15) & ~(size_t)15);
  } else if (strcmp(what, "sup") == 0) {
    int R, cin, res, ws;
    unsigned flags;
    if (sscanf(args, "%d %d %d %d %u", &R, &cin, &res, &ws, &flags) != 5) return false;
    fprintf(f, "%d\n", (!res || x6_bnbwd_takes_residual(R, cin, ws != 0, flags)) ? 1 : 0);
  } else {
    return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: x6_plan_dump cases.txt\n"); return 2; }
  FILE* in = fopen(argv[1], "r");
  if (!in) { perror(argv[1]); return 2; }
  static char line[1 << 16];
  while (fgets(line, sizeof line, in)) {
    line[strcspn(line, "\r\n")] = 0;
    if (line[0] == 0 || line[0] == '#') continue;
    bool ok = false;
    if (strncmp(line, "g ", 2) == 0) ok = dump_gemm(stdout, line + 2);
    else if (strncmp(line, "wb ", 3) == 0) ok = dump_batch(stdout, line + 3);
    else if (strncmp(line, "w ", 2) == 0) ok = dump_wgrad(stdout, line + 2);
    else if (strncmp(line, "q ", 2) == 0) ok = dump_query(stdout, line + 2);
    if (!ok) { fprintf(stderr, "bad case line: %s\n", line); return 2; }
  }
  fclose(in);
  return 0;
}
