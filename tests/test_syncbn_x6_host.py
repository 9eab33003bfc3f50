"""Host side of the fp64 SyncBatchNorm path (no GPU): the five exports are declared in include/gkg_hip.h with the argument lists the
binding derives from it, and the eligibility rules of gkgnet_amd/fused.py let a layer with a statistics group onto the x6 kernels —
except under GKG_DETERMINISTIC and GKG_GEMM_MATH=vendor."""
import ctypes as C

import pytest
import torch

V, I, Z, F = C.c_void_p, C.c_int, C.c_size_t, C.c_float
_TRAIN = [V] * 14 + [I, I, I, I, Z, I, I, I, V, I, F, F, V, Z]               # gkg_bn_apply_train up to zero_doubles
_DUAL = [V] * 15 + [I, I, I, F, F, V, Z]
_PREP = [V] * 13 + [I] * 11 + [C.c_uint, I, I, V, V, V, Z, F, F, V, Z]
_BWD_HEAD = [V] * 6
SYNC_EXPORTS = {
    "gkg_bn_apply_train_sync": _TRAIN + [V, V, V],                           # + count, count_out, stream
    "gkg_bn_apply_train_dual_sync": _DUAL + [V, V, V],
    "gkg_bn_apply_knn_prep_sync": _PREP + [V, V, V],
    "gkg_bn_bwd_stats_f64": _BWD_HEAD + [I, I, I, I, Z, I, V, V, I, V],
    "gkg_bn_bwd_apply_sync": _BWD_HEAD + [V, V, V, I, I, I, I, Z, I, V, V, V, V, Z, V, I, V],
}


def test_header_declares_the_sync_exports():
    from gkgnet_amd import _abi, _lib
    protos = _abi.header().protos
    for name, args in SYNC_EXPORTS.items():
        assert name in protos and name in _lib.EXPORTS, name
        restype, argtypes = protos[name]
        assert restype is I and argtypes == args, (name, len(argtypes), len(args))
    # each _sync form is its local sibling plus (count, count_out) in front of the stream
    for sib in ("gkg_bn_apply_train", "gkg_bn_apply_train_dual", "gkg_bn_apply_knn_prep"):
        assert protos[sib + "_sync"][1] == protos[sib][1][:-1] + [V, V, V], sib
    assert _lib.ABI_VERSION >= 13
    lib = _lib.load()
    for name, args in SYNC_EXPORTS.items():
        assert getattr(lib, name).argtypes == args


class _Group:
    """Stands in for a process group: fused._sync_group is monkeypatched to return it."""


def _layer():
    bn = torch.nn.BatchNorm1d(64).train()
    return torch.zeros(200, 32), torch.zeros(64, 32), bn


def test_a_sync_group_no_longer_keeps_a_layer_off_the_x6_kernels(monkeypatch):
    from gkgnet_amd import _lib, fused
    x, w, bn = _layer()
    monkeypatch.setattr(fused, "GEMM_MATH", "x6")
    monkeypatch.setattr(fused, "DETERMINISTIC", False)
    assert fused._sync_group(bn) is None                       # no process group here: local statistics
    local = (fused._x6(x, w, bn, 1, "fwd"), fused._x6(x, w, bn, 1, "dgrad"), fused._derive_ok(bn, 1, 64, _lib.F32, False))
    assert local == (True, True, True)
    monkeypatch.setattr(fused, "_sync_group", lambda bn_: _Group)
    assert fused._x6(x, w, bn, 1, "fwd") and fused._x6(x, w, bn, 1, "dgrad")
    assert fused._derive_ok(bn, 1, 64, _lib.F32, False)
    assert fused._bn_scale_in_kernel((_Group, None), 1, 64)
    # the count rides behind the sums: one double more than the local form asks of the scratch
    full = fused._BnScratch.DOUBLES // 2
    assert fused._derive_ok(bn, 1, full - 4, _lib.F32, False) and not fused._derive_ok(bn, 1, full, _lib.F32, False)
    # what hands statistics from one node to another stays rank-local
    assert not fused._bwd_fuse_ok(torch.zeros(64), (_Group, None), None, 1, 64)


@pytest.mark.parametrize("switch,value", [("DETERMINISTIC", True), ("GEMM_MATH", "vendor")])
def test_deterministic_and_vendor_keep_the_two_stage_exchange(monkeypatch, switch, value):
    from gkgnet_amd import _lib, fused
    x, w, bn = _layer()
    monkeypatch.setattr(fused, "GEMM_MATH", "x6")
    monkeypatch.setattr(fused, "DETERMINISTIC", False)
    monkeypatch.setattr(fused, "_sync_group", lambda bn_: _Group)
    monkeypatch.setattr(fused, switch, value)
    assert not fused._x6(x, w, bn, 1, "fwd") and not fused._x6(x, w, bn, 1, "dgrad")
    assert not fused._derive_ok(bn, 1, 64, _lib.F32, False)
    assert not fused._bn_scale_in_kernel((_Group, None), 1, 64)
