"""The k-NN launch plan (csrc/gkg_knn_plan.h: knn_plan, pure host code) held to a recorded grid of calls, on the CPU.

tests/knn_plan/plan_dump.cpp, a stand-alone host program, prints the plan of every call in tests/knn_plan/cases.txt (bench and test
shapes under every role and flag set, one case on each side of every comparison constant of the policy, the rejected combinations).
tests/knn_plan/expected.txt is what the library decided for those calls BEFORE the plan had an owner: recorded from the launch
sites of the previous host path (knn_fwd_impl and the per-unit launchers with the HIP runtime calls answered by hipSuccess), printed
by the same formatter.  A threshold edit that moves any case onto another kernel, grid, LDS size or workspace layout shows here."""
import functools
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "knn_plan")
NORM, BF16, DIRECT, BUFFERED, X_PREPARED, Y_PREPARED = 1, 2, 4, 8, 128, 256
FIELDS = "role B G c N M k d dtype flags has_y has_rp ldx xchunk fused".split()


@functools.lru_cache(maxsize=None)
def _dump_exe(tmp):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp, "plan_dump")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gkgnet_amd", "csrc"), os.path.join(HERE, "plan_dump.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _dump_exe(str(tmp_path_factory.mktemp("knn_plan")))


def _run(exe, case_file):
    return subprocess.run([exe, case_file], capture_output=True, text=True, check=True).stdout


def _cases(path):
    out = []
    for line in open(path):
        if line.strip() and not line.startswith("#"):
            t = line.split()
            out.append(dict(zip(FIELDS, [t[0]] + [int(v) for v in t[1:]])))
    return out


def _parse(case_file, text):
    """-> list of (case dict, result dict): line i of the output is case i (format: plan_dump.cpp).  The result has rc (and msg), or
    the plan's fields; tile / pfk / rp as int tuples, off = the hash of the workspace offsets."""
    cases, lines = _cases(case_file), text.splitlines()
    assert len(cases) == len(lines)
    out = []
    for case, line in zip(cases, lines):
        if line in ("ok", "no"):
            res = dict(rc=0 if line == "ok" else -3)
        elif line.startswith("E "):
            res = dict(rc=int(line.split()[1]), msg=line.split(" ", 2)[2])
        else:
            head, _, rest = line.partition(" W ")
            h = head.split()
            res = dict(zip("kd KD S tps cp16 cp16p Nr Mr cpad_ws cpad el".split(), (int(v) for v in h[:11])), rc=0)
            res.update(norm=int(h[11][0]), pf=int(h[11][1]), prep=h[11][2:])
            w, _, rest = rest.partition(" T ")
            off, total = w.split()
            res.update(off=off, total=int(total))
            if rest:
                t, _, pf = rest.partition(" P ")
                t = [int(v) for v in t.split()]
                res.update(tile=tuple(t[:5]) + (res["el"],), lds_tile=t[5], grid=t[6], rp=(t[7], t[8]))
                if pf:
                    v = pf.split()
                    res.update(pfk=(int(v[0]), int(v[1]), int(v[2])), lds_pf=int(v[3]), margin=float(v[4]))
        out.append((case, res))
    return out


@pytest.fixture(scope="module")
def plans(exe):
    return _parse(os.path.join(HERE, "cases.txt"), _run(exe, os.path.join(HERE, "cases.txt")))


def _line(case):
    return " ".join(str(case[f]) for f in FIELDS)


def _launches(case, res):
    return res["rc"] == 0 and case["role"] in ("cm", "tm", "tm16", "fused")


def test_plans_equal_the_recorded_decisions(exe):
    got = _run(exe, os.path.join(HERE, "cases.txt")).splitlines()
    want = open(os.path.join(HERE, "expected.txt")).read().splitlines()
    assert len(got) == len(want) > 1000
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]          # i: index into the case list
    assert not diff, diff[:5]


# The claims of tests/test_hip_knn_bf16_abi.py's docstring about where its FORMS land: (shape, extra flags) -> plan fields.
# tile = (KU, guard, buffer entries, waves, fused aggregation, element); rp = (map, group)
BF16_CLAIMS = [
    ((2, 1, 12, 77, None, 3, 2, True), 0, dict(cp16=16, S=1, tps=3, KD=9, buf=0, grid=2 * 8)),                  # direct by rule; 2 query tiles
    ((2, 4, 80, 324, None, 9, 1, True), 0, dict(S=2, tps=6, grid=48)),                                          # 48 workgroups, 11 key tiles
    ((2, 2, 40, 80, 1000, 9, 1, False), 0, dict(S=4, tps=8, KD=9, buf=12, waves=4)),                            # buffered by rule
    ((8, 1, 40, 4100, 300, 9, 2, True), 0, dict(cp16=48, rp=(1, 1), grid=72 * 8, waves=4, KD=18, buf=16)),      # bias-major map, padded grid
    ((32, 1, 12, 4100, 520, 9, 1, True), 0, dict(waves=1, rp=(1, 1), buf=12, KD=9)),                            # solo AND bias-major; 12 entries
    ((32, 1, 12, 4100, 520, 18, 1, False), 0, dict(waves=1, KD=18, buf=16, rp=(0, 1))),                         # solo, problem-major
    ((1, 2, 200, 300, None, 9, 2, True), 0, dict(cp16=208, KD=18, S=2, tps=5, buf=0)),                          # (short stream: direct by rule)
    ((1, 2, 200, 300, None, 9, 2, True), BUFFERED, dict(KD=18, buf=12, S=2)),                                   # room for 12 entries only
    ((1, 1, 320, 200, None, 9, 3, True), 0, dict(KD=27, tps=7, buf=0)),                                         # direct by rule: short stream
    ((1, 1, 320, 200, None, 9, 3, True), BUFFERED, dict(KD=27, buf=16)),                                        # ... the forced form takes 16
    ((1, 1, 320, 200, None, 9, 2, True), 0, dict(KD=18, buf=0)),                                                # no room for any buffer
    ((1, 1, 320, 200, None, 9, 2, True), BUFFERED, dict(KD=18, buf=12, lds_tile=66 * 1024)),                    # forced: 12 entries, 66 KB
    ((2, 1, 48, 300, None, 18, 2, True), 0, dict(KD=36, S=2)),
    ((1, 1, 16, 100, 333, 32, 2, False), 0, dict(KD=64, S=2, buf=0)),                                           # KD 64: direct only,
    ((1, 1, 16, 100, 333, 32, 2, False), BUFFERED, dict(KD=64, buf=0)),                                         # whatever the flag
    ((1, 1, 33, 65, 130, 5, 1, True), 0, dict(cp16=48, grid=2 * 8, KD=9)),                                      # a second query tile of one row
]


def test_bf16_forms_reach_the_kernels_their_test_claims(plans):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import knn_bf16_ref
    assert {c[0] for c in BF16_CLAIMS} == set(knn_bf16_ref.FORMS)                       # the twelve, each at least once
    by_line = {_line(c): r for c, r in plans}
    for (B, G, c, N, M, k, d, bias), extra, claim in BF16_CLAIMS:
        line = f"tm {B} {G} {c} {N} {N if M is None else M} {k} {d} 0 {NORM | BF16 | extra} {int(M is not None)} {int(bias)} 0 0 0"
        r = by_line[line]
        assert r["rc"] == 0 and r["el"] == 1, line
        got = dict(r, buf=r["tile"][2], waves=r["tile"][3])
        assert {f: got[f] for f in claim} == claim, line
        assert (r["tile"][1] == 1) == (r["tile"][2] == 0), line                         # direct form: the guarded insert


def test_producers_and_consumers_plan_the_same_problem(exe, plans, tmp_path):
    """A producer call (BN-apply producers, the bf16 projection's plan request) and the k-NN call that consumes its work — the same
    problem plus the _PREPARED bit — agree on everything the producer writes: padding, normalisation, prefilter planes, offsets."""
    prod = [(c, r) for c, r in plans if c["role"] in ("prodq", "prodk", "planq") and r["rc"] == 0]
    assert len(prod) > 100 and {c["role"] for c, _ in prod} == {"prodq", "prodk", "planq"}
    cons = []
    for c, _ in prod:
        bit = Y_PREPARED if c["role"] == "prodk" else X_PREPARED
        cons.append(dict(c, role="fused" if c["fused"] else "tm", flags=c["flags"] | bit, fused=0))
    cf = tmp_path / "consumers.txt"
    cf.write_text("\n".join(_line(c) for c in cons) + "\n")
    got = _parse(str(cf), _run(exe, str(cf)))
    assert len(got) == len(prod)
    for (pc, pr), (cc, cr) in zip(prod, got):
        assert cr["rc"] == 0, (pc, cr)
        for f in ("cpad_ws", "cpad", "norm", "pf", "cp16", "cp16p", "Nr", "Mr", "S", "off", "total", "el"):
            assert pr[f] == cr[f], (f, pc, pr, cr)
        # the consumer prepares what is left: nothing of the producer's operand
        assert cr["prep"][1 if pc["role"] == "prodk" else 0] == "0", (pc, cr)
        assert pr["prep"] == {"prodq": "10", "prodk": "01", "planq": "00"}[pc["role"]]
        if pc["fused"]:
            assert cr["tile"][4] == 1, (pc, cr)


def test_workspace_budget_covers_every_plan(plans):
    from gkgnet_amd import _lib
    lib = _lib.load()
    seen = set()
    for c, r in plans:
        if r["rc"] != 0 or "total" not in r:
            continue
        seen.add(c["has_y"])
        budget = lib.gkg_knn_workspace_bytes(c["B"] * c["G"], c["c"], c["N"], c["M"], c["k"], c["d"], c["dtype"], c["flags"])
        assert budget >= r["total"] > 0, (c, budget, r["total"])
        assert r["cpad"] <= r["cpad_ws"] and r["cpad_ws"] % 8 == 0, (c, r)
    assert seen == {0, 1}                                                               # with and without keys


def test_every_planned_form_is_a_kernel_of_the_library(plans):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gkgnet_amd import _build
    # template arguments from the (Itanium-mangled) symbols: knn_tile_kernelILi9ELb1ELi8ELb0ELi16ELi0ELi4ELb0EE -> (9, 1, 8, 0, 16, 0, 4, 0)
    have = set()
    for n in kernel_meta.kernels(_build.build()):
        m = re.search(r"knn_(tile|pf)_kernelI((?:L[ib]\d+E)+)E", n)
        if m:
            have.add((m.group(1),) + tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2))))
    assert len(have) > 150
    want = set()
    for c, r in plans:
        if not _launches(c, r):
            continue
        ku, guard, buf, waves, mrf, el = r["tile"]
        want.add(("tile", r["KD"], c["has_rp"], ku, guard, buf, el, waves, mrf))        # knn_tile_kernel<KD, HAS_RP, KU, GUARD, BUF, BF, NWV, MRF>
        if r["pf"]:
            kdw, pbuf, sb = r["pfk"]
            want.add(("pf", r["KD"], kdw, c["has_rp"], pbuf, sb))                       # knn_pf_kernel<KD, KDW, HAS_RP, PBUF, SB>
    assert len(want) > 100
    assert want <= have, sorted(want - have)
