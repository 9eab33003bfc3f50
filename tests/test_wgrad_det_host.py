"""The run-independent x6 weight gradients (gkg_linear_wgrad_x6_det, GKG_ENABLE=wgrad_det), the parts that need no device: ABI and
exports, the switch's parsing and the two predicates, and the slab plan / workspace size the library reports as pure host code."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import pytest
import torch

from gkgnet_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gkg_linear_wgrad_x6_det", "gkg_linear_wgrad_x6_det_workspace_bytes", "gkg_linear_wgrad_x6_det_slabs",
       "gkg_linear_wgrad_x6_batch_det", "gkg_linear_wgrad_x6_batch_det_workspace_bytes")
CAP = 8192


def test_header_binding_and_library_agree_on_abi_20_and_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "gkg_hip.h")).read()
    m = re.search(r"#define GKG_ABI_VERSION (\d+)", text)
    assert m and int(m.group(1)) == _lib.ABI_VERSION >= 20
    lib = _lib.load()
    assert lib.gkg_version() == _lib.ABI_VERSION
    protos = _abi.header().protos
    for name in NEW:
        assert name in protos and name in _lib.EXPORTS, name
        assert getattr(lib, name).argtypes is not None
    assert protos["gkg_linear_wgrad_x6_det_workspace_bytes"][0] is ctypes.c_size_t
    assert protos["gkg_linear_wgrad_x6_batch_det_workspace_bytes"][0] is ctypes.c_size_t
    assert len(protos["gkg_linear_wgrad_x6_det"][1]) == 16 and len(protos["gkg_linear_wgrad_x6_batch_det"][1]) == 6
    assert _lib._K["ERR_WORKSPACE"] == -4


@pytest.mark.parametrize("env,det,want", [("", "1", "False"), ("wgrad_det", "1", "True"), ("knn_f16, wgrad_det", "0", "True")])
def test_gkg_enable_parsing(env, det, want):
    out = subprocess.run([sys.executable, "-c", "from gkgnet_amd import fused; print(fused.WGRAD_DET)"], cwd=ROOT,
                         env=dict(os.environ, GKG_ENABLE=env, GKG_DETERMINISTIC=det), capture_output=True, text=True, check=True).stdout
    assert out.split() == [want]


def test_switch_is_off_by_default_and_documented():
    from gkgnet_amd import fused
    if "wgrad_det" not in os.environ.get("GKG_ENABLE", ""):
        assert fused.WGRAD_DET is False
    assert "wgrad_det" in open(fused.__file__).read().split("_DISABLED = _env_list")[0]      # the GKG_ENABLE comment table


@pytest.mark.parametrize("det,sw", list(itertools.product((False, True), repeat=2)))
def test_the_two_predicates(monkeypatch, det, sw):
    from gkgnet_amd import fused
    monkeypatch.setattr(fused, "GEMM_MATH", "x6")
    monkeypatch.setattr(fused, "DETERMINISTIC", det)
    monkeypatch.setattr(fused, "WGRAD_DET", sw)
    dY, x = torch.zeros(256, 8), torch.zeros(256, 12)
    assert fused._x6_wgrad_det_ok(dY, x) is (det and sw)
    assert fused._x6_wgrad_ok(dY, x) is (not det)                    # the atomic kernels: never under GKG_DETERMINISTIC
    assert fused._x6_wgrad_det_ok(dY.double(), x) is False and fused._x6_wgrad_det_ok(dY, x, 65) is False
    monkeypatch.setattr(fused, "GEMM_MATH", "vendor")
    assert fused._x6_wgrad_det_ok(dY, x) is False


def test_the_queue_opens_under_deterministic_only_with_the_switch(monkeypatch):
    from gkgnet_amd import fused
    opened = []

    class Q:
        def task_id(self):
            return 7

        def open(self, task, device, units=0, det=False):
            opened.append((task, device, det))
            return self
    monkeypatch.setattr(fused, "_WQ", Q())
    monkeypatch.setattr(fused, "GEMM_MATH", "x6")
    monkeypatch.setattr(fused, "WGRAD_BATCH", True)
    for det, sw, want in ((False, False, False), (False, True, False), (True, False, None), (True, True, True)):
        monkeypatch.setattr(fused, "DETERMINISTIC", det)
        monkeypatch.setattr(fused, "WGRAD_DET", sw)
        del opened[:]
        q = fused._wgrad_queue("dev")
        if want is None:
            assert q is None and not opened
        else:
            assert q is not None and opened == [(7, "dev", want)]


def _slabs(lib, R, cin, cout, nb, ldg, ldx, aligned, ups, slabs):
    first, rows = (ctypes.c_int * CAP)(), (ctypes.c_int * CAP)()
    n = lib.gkg_linear_wgrad_x6_det_slabs(R, cin, cout, nb, ldg, ldx, aligned, ups, slabs, first, rows, CAP)
    return n, list(first[:max(n, 0)]), list(rows[:max(n, 0)])


GRID = [(R, cin, cout, nb) for R in (1, 19, 127, 128, 129, 777, 1000, 1408, 4100, 10368, 663552)
        for cin, cout, nb in ((40, 72, 1), (256, 100, 1), (320, 256, 1), (24, 40, 4), (37, 5, 2), (160, 80, 1))]


@pytest.mark.parametrize("R,cin,cout,nb", GRID)
def test_slab_plan_tiles_the_rows_once_in_order(R, cin, cout, nb):
    lib = _lib.load()
    for aligned, slabs, ups in itertools.product((0, 1), (0, 1, 3, 8, 4096), (0, 2, 20)):
        if ups and slabs:
            continue
        n, first, rows = _slabs(lib, R, cin, cout, nb, cout, cin, aligned, ups, slabs)
        assert 1 <= n <= CAP, (aligned, slabs, ups, n)
        # the slabs tile [0, R) exactly once, in ascending order
        at = 0
        for f, r in zip(first, rows):
            assert f == at and r > 0
            at += r
        assert at == R
        # main slabs (16-byte aligned rows only): whole 128-row units, sizes differing by at most one unit, larger first
        is_al = bool(aligned) and cin % 4 == 0 and cout % 4 == 0
        units = R // 128 if is_al else 0
        main = [r for f, r in zip(first, rows) if f + r <= units * 128]
        assert sum(main) == units * 128 and all(r % 128 == 0 for r in main)
        if main:
            assert max(main) - min(main) <= 128 and main == sorted(main, reverse=True)
        if slabs and not ups:
            assert len(main) == min(slabs, units)
        # every remainder slab but the last is whole 128-row units too
        rest = rows[len(main):]
        assert all(r % 128 == 0 for r in rest[:-1])
        if not ups:
            need = lib.gkg_linear_wgrad_x6_det_workspace_bytes(R, cin, cout, nb, cout, cin, slabs)
            assert need >= n * nb * cout * cin * 4 and need % 16 == 0
        if ups:
            # the batch query agrees with the per-problem plan (aligned operands)
            p = _lib.WgradProblem(0x1000, 0x2000 if aligned else 0x2004, 0x3000, R * cout, R * cin, cout, cin, R, cin, cout, nb, 0)
            arr = (_lib.WgradProblem * 1)(p)
            need = lib.gkg_linear_wgrad_x6_batch_det_workspace_bytes(arr, 1, ups)
            assert need == (n * nb * cout * cin * 4 + 15) // 16 * 16


def test_queries_answer_zero_or_an_error_where_the_call_would_fail():
    lib = _lib.load()
    q, s = lib.gkg_linear_wgrad_x6_det_workspace_bytes, lib.gkg_linear_wgrad_x6_det_slabs
    good = (1024, 40, 72, 1, 72, 40)
    assert q(*good, 0) > 0 and s(*good, 1, 0, 0, None, None, 0) > 0             # cap 0: the count alone
    for bad in ((0, 40, 72, 1, 72, 40), (1024, 0, 72, 1, 72, 40), (1024, 40, 0, 1, 72, 40), (1024, 40, 72, 0, 72, 40),
                (1024, 40, 72, 65, 72, 40), (1024, 40, 72, 1, 71, 40), (1024, 40, 72, 1, 72, 39), (1024, 40, 72, 1, 1 << 26, 40)):
        assert q(*bad, 0) == 0, bad
        assert s(*bad, 1, 0, 0, None, None, 0) < 0, bad
    assert q(*good, -1) == 0 and q(*good, 4097) == 0
    assert s(*good, 1, 0, -1, None, None, 0) == -2 and s(*good, 1, -1, 0, None, None, 0) == -2
    assert s(*good, 1, 0, 0, None, None, 4) == -1                               # a capacity without arrays
    # the calls themselves: argument errors come before anything touches a device
    assert lib.gkg_linear_wgrad_x6_det(None, 72, 0, None, 40, 0, None, *good[:4], 0, 0, None, 0, None) == -1
    assert lib.gkg_linear_wgrad_x6_det(0x1000, 72, 0, 0x2000, 40, 0, 0x3000, 0, 40, 72, 1, 0, 0, 0x4000, 1 << 30, None) == -2
    assert lib.gkg_linear_wgrad_x6_det(0x1000, 72, 0, 0x2000, 40, 0, 0x3000, 1024, 40, 72, 65, 0, 0, 0x4000, 1 << 30, None) == -2
    assert lib.gkg_linear_wgrad_x6_det(0x1000, 72, 0, 0x2000, 41, 0, 0x3000, 1024, 41, 72, 1, 1, 0, 0x4000, 1 << 30, None) == -2
    for ws, nbytes in ((None, 1 << 30), (0x4000, q(*good, 0) - 16), (0x4004, 1 << 30)):
        assert lib.gkg_linear_wgrad_x6_det(0x1000, 72, 0, 0x2000, 40, 0, 0x3000, *good[:4], 0, 0, ws, nbytes, None) == -4
        assert b"workspace" in lib.gkg_last_error_string()
    assert lib.gkg_linear_wgrad_x6_batch_det(None, 0, 0, None, 0, None) == -1
    assert lib.gkg_linear_wgrad_x6_batch_det_workspace_bytes(None, 0, 0) == 0
    p = _lib.WgradProblem(0x1000, 0x2000, 0x3000, 0, 0, 72, 40, 1024, 40, 72, 1, 0)
    arr = (_lib.WgradProblem * 1)(p)
    need = lib.gkg_linear_wgrad_x6_batch_det_workspace_bytes(arr, 1, 2)
    assert need >= 4 * 72 * 40 * 4
    assert lib.gkg_linear_wgrad_x6_batch_det(arr, 1, 2, 0x4000, need - 16, None) == -4
    assert lib.gkg_linear_wgrad_x6_batch_det(arr, 1, 2, None, need, None) == -4
    assert lib.gkg_linear_wgrad_x6_batch_det(arr, 1, 4097, 0x4000, need, None) == -2
    bad = (_lib.WgradProblem * 2)(p, _lib.WgradProblem(0x1000, 0x2000, 0x3000, 0, 0, 72, 40, 0, 40, 72, 1, 0))
    assert lib.gkg_linear_wgrad_x6_batch_det_workspace_bytes(bad, 2, 2) == 0
    assert lib.gkg_linear_wgrad_x6_batch_det(bad, 2, 2, 0x4000, 1 << 30, None) == -2       # the second problem's R: nothing launched
