"""The max-relative aggregation's launch plans (csrc/gkg_mr_plan.h: mr_bwd_tm_plan, mr_fwd_tm_plan, mr_cm_plan, pure host code) held to
a recorded grid of calls, on the CPU.

tests/mr_plan/mr_plan_dump.cpp, a stand-alone host program, prints the plan of every call in tests/mr_plan/cases.txt (mr_ref.BWD_TM
and SHAPES_TM / SHAPES_CM, the stage shapes of bench.py's configurations and of the 576-pixel model under the public flags and every
measurement setting of tools/bench_mr_bwd.py, one case on each side of every comparison constant of the policy, every rejection).
tests/mr_plan/expected.txt is what the library decided for those calls BEFORE the plan had an owner.  Recording method: a scratch
copy of the host half of csrc/gkg_mr.hip at commit ebf6e15 (the entry points, mr_bwd_tm_impl and its launchers, verbatim), compiled
for the CPU with every kernel replaced by a host stub that records its template arguments and arguments at the launch site, the
launch macro recording grid, block and dynamic LDS bytes, GkgProfScope recording the work, gkg_fail the code and message, and the
HIP runtime calls (hipFuncSetAttribute, hipMemsetAsync, hipGetLastError) answered by hipSuccess; driven through the C ABI with dummy
non-null pointers and printed by the same formatter.  A threshold edit that moves any case onto another kernel, chunk width, grid or
LDS size shows here."""
import functools
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "mr_plan")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mr_ref as R                                                                          # noqa: E402

R_ERR_SHAPE = -2                                                                            # GKG_ERR_SHAPE
FIELDS = "fam B G c N M k mode ak flags self stats dtype ldx xchunk alias argmax".split()
FORMS = {"stream": "stream", "stream-f64": "stream-f64", "two-sweep": "two-sweep", "det-private": "private", "det-walk": "walk",
         "lds-f32": "lds-f32", "global-f32": "global-f32"}                                  # plan name -> mr_ref.bwd_form name


@functools.lru_cache(maxsize=None)
def _dump_exe(tmp):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp, "mr_plan_dump")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gkgnet_amd", "csrc"), os.path.join(HERE, "mr_plan_dump.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _dump_exe(str(tmp_path_factory.mktemp("mr_plan")))


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
    """-> list of (case dict, result dict): line i of the output is case i (format: mr_plan_dump.cpp).  The result has rc (and msg), or
    the plan's fields as ints (bwd: form is the plan's name, tmpl = (NT, ACC, U) for the streaming forms)."""
    cases, lines = _cases(case_file), text.splitlines()
    assert len(cases) == len(lines)
    out = []
    for case, line in zip(cases, lines):
        t = line.split()
        if t[0] == "E":
            res = dict(rc=int(t[1]), msg=line.split(" ", 2)[2])
        elif case["fam"] == "bwd":
            res = dict(rc=0, form=t[0], tmpl=None)
            if t[0] in ("stream", "stream-f64"):
                res["tmpl"], t = tuple(int(v) for v in t[1:4]), t[:1] + t[4:]
            res.update(zip("stats cw grid_x grid_y block lds shmax seed_grid gsrc_bytes work".split(), (int(v) for v in t[1:])))
        elif case["fam"] in ("fwd", "fwd16"):
            res = dict(zip("ldx lds schunk write_x grid_x KS AK bf16 work".split(), (int(v) for v in t)), rc=0)
        else:
            res = dict(zip("fallback CH grid_x grid_y grid_z lds seed_grid gsrc_bytes".split(), (int(v) for v in t)), rc=0)
        out.append((case, res))
    return out


def _line(case):
    return " ".join(str(case[f]) for f in FIELDS)


@pytest.fixture(scope="module")
def plans(exe):
    return _parse(os.path.join(HERE, "cases.txt"), _run(exe, os.path.join(HERE, "cases.txt")))


@pytest.fixture(scope="module")
def stats_plans(exe, plans, tmp_path_factory):
    """Every backward case once more with statistics asked (each distinct call once)."""
    asked = sorted({_line(dict(c, stats=1)) for c, _ in plans if c["fam"] == "bwd"})
    cf = tmp_path_factory.mktemp("mr_plan_stats") / "stats.txt"
    cf.write_text("\n".join(asked) + "\n")
    return _parse(str(cf), _run(exe, str(cf)))


def test_plans_equal_the_recorded_decisions(exe):
    got = _run(exe, os.path.join(HERE, "cases.txt")).splitlines()
    want = open(os.path.join(HERE, "expected.txt")).read().splitlines()
    assert len(got) == len(want) > 1000
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]          # i: index into the case list
    assert not diff, diff[:5]


def test_the_grid_reaches_every_form_and_every_rejection(plans):
    assert {r["form"] for c, r in plans if c["fam"] == "bwd" and r["rc"] == 0} == set(FORMS)
    assert {r["tmpl"] for c, r in plans if r.get("tmpl")} == {(512, 0, 4), (512, 0, 8), (256, 0, 4), (256, 0, 8), (512, 1, 4)}
    assert {(r["form"], r["stats"]) for c, r in plans if c["fam"] == "bwd" and r["rc"] == 0 and r["stats"]} == {("stream", 1), ("two-sweep", 1)}
    said = set(re.findall(r'"(gkg_mr_[^"]+)"', open(os.path.join(ROOT, "gkgnet_amd", "csrc", "gkg_mr_plan.h")).read()))
    assert len(said) == 30 and said == {r["msg"] for _, r in plans if r["rc"] != 0}


def test_supported_probe_is_the_plans_answer(stats_plans):
    from gkgnet_amd import _lib
    lib = _lib.load()
    seen = set()
    for c, r in stats_plans:
        got = lib.gkg_mr_bwd_tm_bnstats_supported(c["B"], c["G"], c["c"], c["N"], c["M"], c["k"], c["mode"], c["ak"], c["self"], c["flags"])
        assert got == int(r["rc"] == 0), (c, r)
        seen.add(got)
    assert seen == {0, 1} and len(stats_plans) > 400


def _restated(c):
    return R.bwd_form(c["B"], c["G"], c["c"], c["N"], c["M"], c["flags"])


def test_restated_rule_of_the_gpu_tests_is_the_plans_rule(plans, stats_plans):
    """mr_ref.bwd_form / bwd_stats_supported — what tests/test_hip_mr_bwd_abi.py asserts its forms from — against the plan: form, chunk
    width (private accumulators: TL), (threads, rows in flight), on every backward case with valid sizes."""
    n = 0
    for c, r in plans:
        if c["fam"] != "bwd" or c["stats"] or r["rc"] == R_ERR_SHAPE:
            continue
        form, cw, detail = _restated(c)
        if r["rc"] != 0:
            assert r["msg"].endswith("B <= 65535") and c["B"] > 65535 or form == "unsupported", (c, r)      # (B on grid.y: not restated)
            continue
        assert FORMS[r["form"]] == form, (c, r, form)
        if form in ("stream", "stream-f64", "two-sweep", "lds-f32"):
            assert r["cw"] == cw, (c, r, cw)
        if form == "private":
            assert r["cw"] == detail, (c, r, detail)
        if r["tmpl"]:
            nt, acc, u = r["tmpl"]
            assert (nt, u) == detail[:2] and acc == (form == "stream-f64") and r["block"] == nt, (c, r, detail)
        n += 1
    assert n > 400
    for c, r in stats_plans:
        if r["rc"] != R_ERR_SHAPE:
            assert R.bwd_stats_supported(c["B"], c["G"], c["c"], c["N"], c["M"], c["mode"], c["flags"]) == (r["rc"] == 0), (c, r)
    by_line = {_line(c): r for c, r in plans}
    for shape, flags, form in R.BWD_TM:                                                   # the table the GPU test runs, as planned
        for B, G, c, N, M, k in R.bwd_variants(shape):
            m1 = (G * c) % 16 == 0
            r = by_line[f"bwd {B} {G} {c} {N} {N if M is None else M} {k} {int(m1)} {int(m1)} {flags} {int(M is None)} 0 0 0 0 0 0"]
            assert r["rc"] == 0 and FORMS[r["form"]] == form, (shape, flags, form, r)



def test_every_planned_form_is_a_kernel_of_the_library(plans):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gkgnet_amd import _build
    # template arguments from the (Itanium-mangled) symbols: mr_bwd_tm_stream_kernelILi512ELb1ELi1ELi0ELi0ELi4ELb1EE -> (512, 1, 1, 0, 0, 4, 1);
    # types: f float, t unsigned short (bf16 / u16 rows), DF16_ _Float16, l int64
    have = set()
    for n in kernel_meta.kernels(_build.build()):
        m = re.search(r"3gkg\d+(mr_\w+?_kernel|negate_kernel)(?:I((?:L[ib]\d+E|DF16_|[ftl])+)E)?E", n)
        if m and not m.group(1).startswith(("mr_fc2", "mr_linear")):
            args = re.findall(r"L[ib](\d+)E|(DF16_|[ftl])", m.group(2) or "")
            have.add((m.group(1),) + tuple(int(a) if a else b for a, b in args))
    assert len(have) == 105
    el = {0: "f", 1: "t", 2: "DF16_"}                                                   # GKG_F32 / GKG_BF16 / GKG_F16
    from gkgnet_amd import _abi
    K = _abi.header().constants
    assert (K["F32"], K["BF16"], K["F16"]) == (0, 1, 2)
    want = set()
    for c, r in plans:
        if r["rc"] != 0:
            continue
        sma = (c["self"], c["mode"], c["ak"])
        if c["fam"] == "bwd":
            if r["seed_grid"]:
                want |= {("mr_bwd_tm_init_kernel",), ("mr_bwd_tm_det_global_kernel" if r["form"] == "det-walk" else "mr_bwd_tm_scatter_atomic_kernel",)}
            elif r["tmpl"]:
                nt, acc, u = r["tmpl"]
                want.add(("mr_bwd_tm_stream_kernel", nt) + sma + (acc, u, r["stats"]))
            elif r["form"] == "two-sweep":
                want.add(("mr_bwd_tm_scatter_i64_kernel",) + sma + (r["stats"],))
            else:
                want.add(({"det-private": "mr_bwd_tm_det_kernel", "lds-f32": "mr_bwd_tm_scatter_kernel"}[r["form"]],) + sma)
        elif c["fam"] in ("fwd", "fwd16"):
            want.add(("mr_fwd_tm_kernel", r["KS"], 1, "t" if r["bf16"] else "f", r["AK"], "t" if c["fam"] == "fwd16" else "l"))
        elif c["fam"] == "cmf":
            want.add(("mr_fwd_gather_kernel" if r["fallback"] else "mr_fwd_kernel", el[c["dtype"]]))
        elif r["fallback"]:
            want |= {("mr_bwd_atomic_kernel",)} | ({("negate_kernel",)} if r["seed_grid"] else set())
        else:
            want.add(("mr_bwd_kernel", el[c["dtype"]], c["self"]))
    assert want <= have, sorted(want - have, key=str)
    assert want == have, sorted(have - want, key=str)                                     # and the grid reaches every kernel of the unit


def test_planned_launches_fit_the_device(plans):
    for c, r in plans:
        if r["rc"] != 0:
            continue
        assert r.get("lds", 0) <= 160 * 1024, (c, r)
        assert 0 < r["grid_x"] <= 0x7FFFFFFF and 0 < r.get("grid_y", 1) <= 65535 and 0 < r.get("grid_z", 1) <= 65535, (c, r)
        assert r.get("block", 256) in (64, 256, 512), (c, r)
        if r.get("seed_grid"):
            assert r["seed_grid"] <= 0x7FFFFFFF, (c, r)
