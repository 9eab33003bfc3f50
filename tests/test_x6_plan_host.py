"""The launch plans of the split-bf16 projection GEMMs and their weight gradients (csrc/gkg_x6_plan.h: x6_gemm_plan, x6_wgrad_plan,
x6_wgrad_batch_plan, pure host code) held to a recorded grid of calls, on the CPU.

tests/x6_plan/x6_plan_dump.cpp, a stand-alone host program, prints the plan of every call in tests/x6_plan/cases.txt: every projection
shape of bench.py's configurations and of the 576-pixel model in all four GEMM roles (forward, input gradient, input gradient stored
channel-major, input gradient with BN-backward statistics) with / without / with a too small split-K workspace, under every GKG_X6_* flag,
two walk caps and three resident-workgroup counts; one case on each side of every comparison constant of the ladder; every rejection;
the same layer shapes as weight gradients stand-alone, deterministic with forced slab counts and batched; the batch assembly (1, 16, 17,
256 problems, 257 rejected, ties, ragged remainders between the group launches); the host-side queries.
tests/x6_plan/expected.txt is what the library decided for those calls BEFORE the plan had an owner.  Recording method: a scratch copy
of the host half of csrc/gkg_gemm_x6.hip at commit 178cb39 (x6_kernel_setup, x6_walk_grid, x6_launch_ni, x6_launch_ks, x6_ks_form,
x6_tile_ksplit, x6_launch, x6_wgrad_plan and every entry point from gkg_linear_bn_fwd_x6 to gkg_linear_wgrad_x6_batch_det, verbatim),
compiled for the CPU with every kernel replaced by a host stub that records its template arguments and the size fields of its argument
struct, the launch macro recording grid, block and dynamic LDS bytes, GkgProfScope the work, gkg_fail the code and message, the HIP
runtime calls answered by hipSuccess and the occupancy query by the case's slots / CUs (one fake device per slots value, since the
count is cached per device); driven through the C ABI with dummy non-null pointers whose alignment the case chooses (each batch
problem's x pointer tells the problems apart in the recorded launches), and printed in the dump program's format.  The short-matrix
body's unread X6Args::ksplit (0 in the parent) is printed as 1.  A threshold edit that moves any case onto another body, tile width,
split, grid, LDS size, slab plan or launch order shows here."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "x6_plan")
PLAN_H = os.path.join(ROOT, "gkgnet_amd", "csrc", "gkg_x6_plan.h")
NO_WALK = 4                                                                                 # GKG_X6_NO_WALK
G_CASE = "role R cin cout nb ws flags res train slots lda abs ldc cbs aal n1 n2 n3".split()
G_PLAN = "body epi NI BN mtiles ntiles ksplit kper grid_x grid_y lds NP KC p_bstride nslots work".split()
W_CASE = "mode val R cin cout nb ldg ldx gbs xbs al kperm".split()


@functools.lru_cache(maxsize=None)
def _dump_exe(tmp):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp, "x6_plan_dump")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gkgnet_amd", "csrc"), os.path.join(HERE, "x6_plan_dump.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _dump_exe(str(tmp_path_factory.mktemp("x6_plan")))


def _run(exe, case_file):
    return subprocess.run([exe, case_file], capture_output=True, text=True, check=True).stdout


def _ints(names, tokens):
    return dict(zip(names, (int(t) for t in tokens)))


def _parse(case_file, text):
    """-> list of (kind, case dict, result dict): line i of the output is case i (formats: x6_plan_dump.cpp).  A result has rc (and msg)
    or the printed fields; wb: `launches`, a list of ("B", n, workgroups, [problem tuples]) / ("R", i, ...) and `ws_bytes` (det)."""
    cases = [ln.split() for ln in open(case_file) if ln.strip() and not ln.startswith("#")]
    lines = text.splitlines()
    assert len(cases) == len(lines)
    out = []
    for t, line in zip(cases, lines):
        kind, r = t[0], line.split()
        if kind == "g":
            case = dict(_ints(G_CASE[1:], t[2:]), role=t[1])
        elif kind == "w":
            case = dict(_ints(W_CASE[1:], t[2:]), mode=t[1])
        elif kind == "wb":
            listed = [tuple(int(v) for v in p.split(",")) for p in t[4:]]                    # a list shorter than n repeats
            case = dict(det=int(t[1]), ups=int(t[2]), n=int(t[3]), problems=[listed[i % len(listed)] for i in range(int(t[3]) if listed else 0)])
        else:
            case = dict(what=t[1], args=[int(v) for v in t[2:]])
        if r[0] == "E":
            res = dict(rc=int(r[1]), msg=line.split(" ", 2)[2])
        elif kind == "g":
            two = r[0] == "2L"
            r = r[1:] if two else r
            res = dict(_ints(G_PLAN[1:], r[1:]), body=r[0], two_launch=two, rc=0)
        elif kind == "w":
            assert r[3] == "M" and r[15] == "R"
            res = dict(rc=0, wide=int(r[0]), swap=int(r[1]), kperm=int(r[2]),
                       main=_ints("rows M N mtiles ntiles splits rows_per_split share ubase urem grid_x".split(), r[4:15]),
                       rest=_ints("rows row0 splits rows_per_split grid_x".split(), r[16:]))
        elif kind == "wb":
            res = dict(rc=0, launches=[], ws_bytes=None)
            for part in line.split(" ; "):
                p = part.split()
                if p[0] == "F":
                    res["ws_bytes"] = int(p[1])
                elif p[0] == "R":
                    res["launches"].append(("R",) + tuple(int(v) for v in p[1:]))
                else:
                    probs = [tuple(int(v) for v in m.replace(" M", "").split()) for m in re.findall(r"\[([^\]]+)\]", part)]
                    assert len(probs) == int(p[1])
                    res["launches"].append(("B", int(p[1]), int(p[2]), probs))
        else:
            res = dict(rc=0, values=[int(v) for v in r])
        out.append((kind, case, res))
    return out


@pytest.fixture(scope="module")
def plans(exe):
    cf = os.path.join(HERE, "cases.txt")
    return _parse(cf, _run(exe, cf))


def test_plans_equal_the_recorded_decisions(exe):
    got = _run(exe, os.path.join(HERE, "cases.txt")).splitlines()
    want = open(os.path.join(HERE, "expected.txt")).read().splitlines()
    assert len(got) == len(want) > 1000
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]          # i: index into the case list
    assert not diff, diff[:5]


def test_the_grid_reaches_every_form_and_every_rejection(plans):
    g = [(c, r) for k, c, r in plans if k == "g" and r["rc"] == 0]
    forms = {(r["body"], r["NI"], r["BN"], r["epi"]) for _, r in g}
    assert forms == ({("ks", 2, 64, e) for e in (0, 1, 2)} | {("tile", 2, 64, e) for e in range(4)} | {("tile", 1, 32, e) for e in range(4)}
                     | {("tile", 3, 80, e) for e in (0, 1)} | {("walk", 2, 64, e) for e in (0, 1, 3)})
    assert {r["ksplit"] for _, r in g} >= {1, 2, 3, 4, 5, 8} and {r["nslots"] for _, r in g} >= {0, 1, 4, 5, 16}
    assert {r["two_launch"] for c, r in g if c["role"] == "nchw"} == {False, True}
    w = [(c, r) for k, c, r in plans if k == "w" and r["rc"] == 0]
    assert {(r["wide"], r["swap"], r["main"]["rows"] > 0, r["rest"]["rows"] > 0) for _, r in w} == {
        (0, 0, True, False), (0, 0, True, True), (0, 0, False, True), (1, 0, True, False), (1, 0, True, True), (1, 1, True, False), (1, 1, True, True)}
    shares = {p[13] for k, c, r in plans if k == "wb" and r["rc"] == 0 for la in r["launches"] if la[0] == "B" for p in la[3]}
    # the fills-the-chip rule on both sides of tiles * stand-alone slabs == 512 (one unit: the slab count is 1)
    one_unit = {(p[9] * p[10], p[13]) for k, c, r in plans if k == "wb" and r["rc"] == 0 for la in r["launches"] if la[0] == "B" for p in la[3] if p[6] == 128}
    assert {(511, 8), (512, 0)} <= one_unit
    assert shares == {0, 2, 4, 8}                                                           # 8 + slabs on their own XCDs, 4 / 2 / 1 slabs shared
    assert {la[1] for k, c, r in plans if k == "wb" and r["rc"] == 0 for la in r["launches"] if la[0] == "B"} >= {1, 8, 16}
    # every message of the plan header is the answer to some case
    said = set(re.findall(r'"(gkg_\w+: [^"]+)"', open(PLAN_H).read()))
    assert len(said) == 27 and said <= {r["msg"] for _, _, r in plans if r["rc"] != 0}, sorted(said - {r["msg"] for _, _, r in plans if r["rc"] != 0})


def _problem_array(problems):
    from gkgnet_amd import _lib
    arr = (_lib.WgradProblem * max(len(problems), 1))()
    for i, (R, cin, cout, nb, ldg, ldx, al, kperm) in enumerate(problems):
        arr[i] = _lib.WgradProblem(0 if al == 2 else 0x10000000 + (0 if al else 4), 0x20000000, 0x40000000 + i * 0x100000, R * ldg, R * ldx, ldg, ldx, R, cin, cout, nb, kperm)
    return arr


def test_query_entry_points_are_the_plans_answers(plans):
    """gkg_linear_wgrad_x6_det_slabs, both *_workspace_bytes and gkg_linear_dgrad_x6_bnbwd_sk_supported of the loaded library against the
    dump program, on every case that asks them.  gkg_x6_walk_workgroups needs a device wherever the resident-workgroup count decides;
    it is held to the plan on the forward cases where it does not (the answer is 0: another body, a split, 32- / 80-column tiles,
    GKG_X6_NO_WALK), and on the others the plan alone is asserted (a walk has a grid of whole XCD rounds)."""
    from gkgnet_amd import _lib
    lib = _lib.load()
    first, rows = (ctypes.c_int * 8192)(), (ctypes.c_int * 8192)()
    n = dict(slabs=0, wsb=0, sup=0, bwsb=0, walk0=0, walk=0)
    for kind, c, r in plans:
        if kind == "q" and c["what"] == "slabs":
            got = lib.gkg_linear_wgrad_x6_det_slabs(*c["args"], first, rows, 8192)
            if r["rc"] != 0:
                assert got == r["rc"], (c, r, got)
                continue
            h = 0
            for s in range(got):
                h = ((h * 31 + first[s]) * 31 + rows[s]) & 0xFFFFFFFF
            assert [got, h] == r["values"], (c, r, got, h)
            n["slabs"] += 1
        elif kind == "q" and c["what"] == "wsb":
            assert lib.gkg_linear_wgrad_x6_det_workspace_bytes(*c["args"]) == r["values"][0], (c, r)
            n["wsb"] += 1
        elif kind == "q" and c["what"] == "sup":
            assert lib.gkg_linear_dgrad_x6_bnbwd_sk_supported(*c["args"]) == r["values"][0], (c, r)
            n["sup"] += 1
        elif kind == "wb" and c["det"] and c["n"] <= 256:
            got = lib.gkg_linear_wgrad_x6_batch_det_workspace_bytes(_problem_array(c["problems"]) if c["n"] else None, c["n"], c["ups"])
            assert got == (r["ws_bytes"] if r["rc"] == 0 else 0), (c, r, got)
            n["bwsb"] += 1
        elif (kind == "g" and c["role"] == "fwd" and c["train"] == 0 and r["rc"] == 0 and c["ws"] in (0, 1) and (c["lda"], c["abs"]) == (0, 0)):
            decided_by_slots = r["body"] == "walk" or ((r["body"], r["NI"], r["ksplit"]) == ("tile", 2, 1) and r["BN"] == 64 and not c["flags"] & NO_WALK)
            if not decided_by_slots:
                assert lib.gkg_x6_walk_workgroups(c["R"], c["cin"], c["cout"], c["nb"], c["ws"], c["flags"]) == 0, (c, r)
                n["walk0"] += 1
            elif r["body"] == "walk":
                assert r["grid_x"] > 0 and r["grid_x"] % 8 == 0 and r["grid_y"] == 1, (c, r)
                n["walk"] += 1
    assert n["slabs"] > 60 and n["wsb"] > 30 and n["sup"] == 108 and n["bwsb"] > 40 and n["walk0"] > 30 and n["walk"] > 15, n      # (the sizes of the grid)


def test_equal_slots_give_equal_walk_grids_for_store_and_bnstats(exe, plans, tmp_path_factory):
    """The walk query asks the device about the X6_STORE instantiation and the training forward launches X6_BNSTATS (2 KiB more LDS): on
    the plan, the same resident-workgroup count gives both epilogues the same body, tiles and grid; only the walk's LDS differs."""
    lines = set()
    for kind, c, r in plans:
        if kind == "g" and c["role"] == "fwd" and r["rc"] == 0 and c["nb"] * 2 * c["cout"] <= 2 * 4096 * 4:
            for train in (0, 2):
                lines.add("g fwd " + " ".join(str(dict(c, train=train)[f]) for f in G_CASE[1:]))
    lines = sorted(lines)
    cf = tmp_path_factory.mktemp("x6_plan_roles") / "roles.txt"
    cf.write_text("\n".join(lines) + "\n")
    by = {}
    for _, c, r in _parse(str(cf), _run(exe, str(cf))):
        assert r["rc"] == 0, (c, r)
        by.setdefault(tuple(c[f] for f in G_CASE if f != "train"), {})[c["train"]] = r
    walks = 0
    for key, pair in by.items():
        s, b = pair[0], pair[2]
        assert (s["epi"], b["epi"]) == (0, 1)
        same = [f for f in G_PLAN if f not in ("epi", "lds", "nslots")]
        assert [s[f] for f in same] == [b[f] for f in same], (key, s, b)
        assert b["lds"] - s["lds"] == (2048 if s["body"] == "walk" else 0), (key, s, b)
        walks += s["body"] == "walk"
    assert len(by) > 200 and walks > 30


def test_every_planned_form_is_a_kernel_of_the_library(plans):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gkgnet_amd import _build
    have = set()
    for name in kernel_meta.kernels(_build.build()):
        m = re.search(r"3gkg\d+((?:gemm|wgrad)_x6_\w*?kernel)(?:I((?:Li\d+E)+)E)?E", name)
        if m:
            have.add((m.group(1),) + tuple(int(a) for a in re.findall(r"Li(\d+)E", m.group(2) or "")))
    assert len(have) == 25, sorted(have)
    want = set()
    for kind, c, r in plans:
        if r["rc"] != 0:
            continue
        if kind == "g":
            want.add({"ks": ("gemm_x6_ks_kernel", r["epi"], 1), "tile": ("gemm_x6_kernel", r["NI"], r["epi"], r["BN"]),
                      "walk": ("gemm_x6_walk_kernel", r["NI"], r["epi"], r["BN"])}[r["body"]])
        elif kind == "w":
            det = "_det" if c["mode"] == "det" else ""
            if r["main"]["rows"]:
                want.add((("wgrad_x6_wide" if r["wide"] else "wgrad_x6_dma") + det + "_kernel",))
            if r["rest"]["rows"]:
                want.add(("wgrad_x6" + det + "_kernel",))
            if det:
                want.add(("wgrad_x6_det_reduce_kernel",))
        elif kind == "wb":
            det = "_det" if c["det"] else ""
            for la in r["launches"]:
                want.add(("wgrad_x6_batch" + det + "_kernel",) if la[0] == "B" else ("wgrad_x6" + det + "_kernel",))
    print(f"x6 kernels reached by the case grid: {len(want & have)} of {len(have)} built")
    assert want <= have, sorted(want - have, key=str)
    assert want == have, sorted(have - want, key=str)                                     # and the grid reaches every x6 kernel of the unit


def test_planned_launches_fit_the_device(plans):
    for kind, c, r in plans:
        if r["rc"] != 0:
            continue
        if kind == "g":
            assert r["lds"] <= 160 * 1024 and 0 < r["grid_x"] <= 0x7FFFFFFF and 0 < r["grid_y"] <= 65535, (c, r)
            assert r["grid_x"] % 8 == 0 and (r["ksplit"] == 1 or r["ksplit"] * r["kper"] >= (c["cin" if c["role"] == "fwd" else "cout"] + 31) // 32), (c, r)
        elif kind == "w":
            assert r["main"]["grid_x"] % 8 == 0 and r["rest"]["grid_x"] % 8 == 0 and r["main"]["rows"] + r["rest"]["rows"] == c["R"], (c, r)
            assert (not r["rest"]["rows"] or r["rest"]["row0"] == r["main"]["rows"]) and r["main"]["rows"] % 128 == 0, (c, r)
        elif kind == "wb":
            for la in r["launches"]:
                assert la[0] == "R" or (0 < la[1] <= 16 and la[2] % 8 == 0 and la[2] == la[3][-1][5]), (c, la)
