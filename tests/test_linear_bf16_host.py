"""gkg_linear_bf16 (csrc/gkg_linear_bf16.hip), the parts that need no device: the three entry points in the header and the derived
binding, the pure host functions, the weight's fragment array, the opt-in switch and the dispatch predicate of ``fused._lin``."""
import ctypes as C
import types

import pytest
import torch

I, P, F = C.c_int, C.c_void_p, C.c_void_p


def test_header_declares_the_three_entry_points():
    from gkgnet_amd import _abi, _lib
    protos = _abi.header().protos
    assert protos["gkg_linear_bf16_supported"] == (I, [I] * 7)
    assert protos["gkg_linear_bf16_planes_bytes"] == (C.c_size_t, [I, I])
    assert protos["gkg_linear_bf16"] == (I, [P, I, P, F, F, F, I, F, I, P, I, I, I, I, I, P])
    for name in ("gkg_linear_bf16_supported", "gkg_linear_bf16_planes_bytes", "gkg_linear_bf16"):
        assert name in _lib.EXPORTS


def test_host_functions_answer_without_a_device():
    from gkgnet_amd import _lib
    lib = _lib.load()
    for R, cin, cout in [(1, 16, 8), (324, 80, 80), (65, 2560, 640)]:
        for has_res, w32, w16, act in [(0, 1, 0, 0), (1, 1, 1, 0), (0, 0, 1, 1), (1, 1, 1, 1)]:
            assert lib.gkg_linear_bf16_supported(R, cin, cout, has_res, w32, w16, act) == 1
    assert lib.gkg_linear_bf16_supported(65, 12, 80, 0, 1, 0, 0) == 0
    assert lib.gkg_linear_bf16_supported(65, 80, 20, 0, 1, 0, 0) == 0
    assert lib.gkg_linear_bf16_supported(0, 80, 80, 0, 1, 0, 0) == 0
    assert lib.gkg_linear_bf16_supported(65, 80, 80, 0, 0, 0, 0) == 0            # no output wanted
    assert lib.gkg_linear_bf16_supported(65, 80, 80, 0, 1, 0, 2) == 0            # unknown activation
    assert lib.gkg_linear_bf16_planes_bytes(12, 80) == 0 and lib.gkg_linear_bf16_planes_bytes(80, 20) == 0
    # the header's paddings: contraction to 16, output columns to 32
    assert lib.gkg_linear_bf16_planes_bytes(24, 40) == (32 // 8) * 64 * 16
    assert lib.gkg_linear_bf16_planes_bytes(2560, 640) == (2560 // 8) * 640 * 16


def test_planes_are_the_fragments_of_the_unfolded_weight_and_cached():
    from gkgnet_amd import _lib, derived
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(24, 40, 1)
    p = derived.lin_planes(conv)
    assert p.dtype == torch.bfloat16 and p.is_contiguous()
    assert p.numel() * 2 == _lib.load().gkg_linear_bf16_planes_bytes(24, 40)
    nf, co_pad, _ = p.shape
    w16 = conv.weight.detach().reshape(40, 24).to(torch.bfloat16)
    for f in range(nf):
        for n in range(co_pad):
            want = torch.zeros(8, dtype=torch.bfloat16)
            if n < 40 and 8 * f < 24:
                want = w16[n, 8 * f:8 * f + 8]
            assert torch.equal(p[f, n], want), (f, n)
    assert (p[3:] == 0).all() and (p[:, 40:] == 0).all()                         # the pad region
    assert derived.lin_planes(conv) is p                                       # cached
    with torch.no_grad():
        conv.weight.mul_(2.0)
    p2 = derived.lin_planes(conv)
    assert p2 is not p and torch.equal(p2[:3, :40].float(), 2.0 * p[:3, :40].float())


def test_switch_is_off_by_default():
    import os
    from gkgnet_amd import fused
    if "lin_bf16" not in os.environ.get("GKG_ENABLE", ""):
        assert fused.LIN_BF16 is False


def _objs(dtype=torch.bfloat16, training=False, groups=1):
    x = types.SimpleNamespace(dtype=dtype, shape=(324, 80))
    conv = types.SimpleNamespace(groups=groups, weight=types.SimpleNamespace(shape=(160, 80 // groups, 1, 1)))
    bn = types.SimpleNamespace(training=training, track_running_stats=True)
    return x, conv, bn


def test_dispatch_predicate_truth_table(monkeypatch):
    """One flipped input per row turns the dispatch off.  Plain Python objects: no CUDA tensor, no autocast context (the two torch
    queries lowp_inference reads are answered by the test)."""
    from gkgnet_amd import fused
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.bfloat16)
    sup = lambda R, cin, cout: (R, cin, cout) == (324, 80, 160)                  # noqa: E731
    ok = fused.lin_bf16_ok
    with torch.no_grad():
        lp = fused.lowp_inference()
    assert lp is True
    x, conv, bn = _objs()
    assert ok(True, lp, x, conv, bn, supported=sup) is True
    assert ok(True, lp, x, conv, bn) is True                                     # the library's own answer (host code)
    assert ok(False, lp, x, conv, bn, supported=sup) is False                    # switch off
    with torch.enable_grad():
        assert ok(True, fused.lowp_inference(), x, conv, bn, supported=sup) is False          # grad enabled
    assert ok(True, lp, _objs(dtype=torch.float32)[0], conv, bn, supported=sup) is False      # fp32 x
    assert ok(True, lp, x, conv, bn, nchw=(2, 160, 18, 18), supported=sup) is False
    assert ok(True, lp, x, conv, bn, scale=object(), supported=sup) is False
    assert ok(True, lp, x, conv, _objs(training=True)[2], supported=sup) is False             # train-mode BN
    assert ok(True, lp, x, _objs(groups=4)[1], bn, supported=sup) is False
    # ... and the rest of the list
    assert ok(True, lp, x, conv, bn, chain=False, supported=sup) is False
    for kw in ("xm", "knn"):
        assert ok(True, lp, x, conv, bn, supported=sup, **{kw: object()}) is False
    for kw in ("alias", "dual"):
        assert ok(True, lp, x, conv, bn, supported=sup, **{kw: True}) is False
    bn2 = types.SimpleNamespace(training=False, track_running_stats=False)
    assert ok(True, lp, x, conv, bn2, supported=sup) is False
    assert ok(True, lp, x, conv, bn, supported=lambda *a: False) is False
    x12 = types.SimpleNamespace(dtype=torch.bfloat16, shape=(324, 12))
    conv12 = types.SimpleNamespace(groups=1, weight=types.SimpleNamespace(shape=(160, 12, 1, 1)))
    assert ok(True, lp, x12, conv12, bn) is False                                # the library says no: cin % 8
