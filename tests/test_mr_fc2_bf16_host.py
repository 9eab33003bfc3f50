"""gkg_mr_fc2_bf16 (csrc/gkg_mr_fc2_bf16.hip), the parts that need no device: the three entry points in the header and the derived
binding, the pure host predicate, the opt-in switch and the dispatch predicate of ``fused.grapher_forward``."""
import ctypes as C
import types

import torch

I, P = C.c_int, C.c_void_p

CALL = [P] * 10 + [I, P, I, P, I] + [I] * 7 + [P]      # x src idx wplanes a1 c1 w2planes a2 c2 res | ldr o32 ldo32 o16 ldo16 | B G c N M k act | stream


def test_header_declares_the_three_entry_points():
    from gkgnet_amd import _abi, _lib
    assert _lib.ABI_VERSION >= 18
    protos = _abi.header().protos
    assert protos["gkg_mr_fc2_bf16_supported"] == (I, [I] * 10)
    assert protos["gkg_mr_fc2_bf16"] == (I, CALL)
    assert protos["gkg_mr_fc2_bf16_nn16"] == (I, CALL)
    for name in ("gkg_mr_fc2_bf16_supported", "gkg_mr_fc2_bf16", "gkg_mr_fc2_bf16_nn16"):
        assert name in _lib.EXPORTS
    lib = _lib.load()
    assert lib.gkg_version() == _lib.ABI_VERSION


def test_host_predicate_answers_without_a_device():
    from gkgnet_amd import _lib
    sup = _lib.load().gkg_mr_fc2_bf16_supported
    # (B, G, c, N, M, k): cfg3 stages 1-2, cfg5 stages 1-2, the smallest
    for shape in [(32, 2, 40, 20736, 1296, 9), (32, 2, 80, 5184, 1296, 9), (16, 8, 12, 36864, 2304, 18), (16, 8, 24, 9216, 2304, 18),
                  (1, 2, 8, 64, 64, 3)]:
        for has_res, w32, w16, act in [(1, 1, 1, 1), (0, 1, 0, 0), (0, 0, 1, 1), (1, 1, 0, 0)]:
            assert sup(*shape, has_res, w32, w16, act) == 1, shape
    assert sup(2, 2, 104, 100, 100, 9, 1, 1, 1, 1) == 0          # C = 208: beyond the envelope
    assert sup(2, 2, 200, 100, 100, 9, 1, 1, 1, 1) == 0          # C = 400
    assert sup(2, 8, 10, 100, 100, 9, 1, 1, 1, 1) == 0           # c % 4 != 0 (C = 80)
    assert sup(2, 2, 40, 100, 100, 65, 1, 1, 1, 1) == 0          # k = 65
    assert sup(2, 2, 40, 100, 100, 9, 1, 0, 0, 1) == 0           # no output wanted
    assert sup(2, 2, 40, 100, 100, 9, 1, 1, 1, 2) == 0           # unknown activation
    assert sup(0, 2, 40, 100, 100, 9, 1, 1, 1, 1) == 0           # B = 0
    assert sup(2, 2, 40, 100, 100, 9, 1, 1, 1, 1) == 1


def test_switch_is_off_by_default_and_documented():
    import os
    from gkgnet_amd import fused
    if "mr_fc2_bf16" not in os.environ.get("GKG_ENABLE", ""):
        assert fused.MR_FC2_BF16 is False
    assert "mr_fc2_bf16" in open(fused.__file__).read().split("_DISABLED = _env_list")[0]      # the GKG_ENABLE comment table


def _layer(cin, cout, training=False, groups=1):
    conv = types.SimpleNamespace(groups=groups, weight=types.SimpleNamespace(shape=(cout, cin // groups, 1, 1)))
    return (conv, types.SimpleNamespace(training=training, track_running_stats=True))


def test_dispatch_predicate_truth_table(monkeypatch):
    """One flipped input per row turns the dispatch off.  Plain Python objects: no CUDA tensor, no autocast context (the two torch
    queries lowp_inference reads are answered by the test)."""
    from gkgnet_amd import fused
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.bfloat16)
    monkeypatch.setattr(fused, "MR_GEMM", True)
    asked = []

    def sup(B, G, c, N, M, k):
        asked.append((B, G, c, N, M, k))
        return (B, G, c, N, M, k) in ((2, 2, 80, 256, 256, 9), (2, 2, 80, 256, 64, 9))
    ok = fused.mr_fc2_bf16_ok
    with torch.no_grad():
        lp = fused.lowp_inference()
    assert lp is True
    F32, NS = torch.float32, types.SimpleNamespace
    x = NS(dtype=F32, shape=(2, 256, 160))
    src = NS(dtype=F32, shape=(2, 64, 160))
    idx = NS(dtype=torch.int16, shape=(4, 256, 9))
    res = NS(dtype=F32, shape=(512, 160))
    nn_, fc2 = _layer(320, 320, groups=4) + (object(),), _layer(320, 160)
    assert ok("all", lp, x, None, idx, 2, nn_, fc2, res, None, True, supported=sup) is True
    assert asked == [(2, 2, 80, 256, 256, 9)]
    assert ok("all", lp, x, src, idx, 2, nn_, fc2, res, None, True, supported=sup) is True             # pooled keys
    assert ok("all", lp, x, None, NS(dtype=torch.int64, shape=(4, 256, 9)), 2, nn_, fc2, res, None, True, supported=sup) is True
    assert ok("all", lp, x, None, idx, 2, nn_, fc2, None, None, True, supported=sup) is True            # no residual
    assert ok("all", lp, x, None, idx, 2, nn_, fc2, res, None, True) is True                            # the library's own answer (host code)
    assert ok(False, lp, x, None, idx, 2, nn_, fc2, res, None, True, supported=sup) is False            # switch off
    with torch.enable_grad():
        assert ok("all", fused.lowp_inference(), x, None, idx, 2, nn_, fc2, res, None, True, supported=sup) is False   # gradients on
    assert ok("all", lp, x, None, idx, 2, nn_, fc2, res, None, False, supported=sup) is False           # off the channels-last chain
    assert ok("all", lp, x, None, idx, 2, _layer(320, 320, True, 4) + (object(),), fc2, res, None, True, supported=sup) is False   # train-mode BN
    assert ok("all", lp, x, None, idx, 2, nn_, _layer(320, 160, training=True), res, None, True, supported=sup) is False
    assert ok("all", lp, x, None, idx, 2, _layer(320, 320, groups=2) + (object(),), fc2, res, None, True, supported=sup) is False  # groups != 4
    assert ok("all", lp, x, None, idx, 2, nn_, _layer(320, 160, groups=4), res, None, True, supported=sup) is False     # a grouped fc2
    assert ok("all", lp, x, None, idx, 2, nn_, fc2, res, object(), True, supported=sup) is False        # a DropPath scale
    assert ok("all", lp, x, None, idx, 2, nn_, fc2, NS(dtype=torch.bfloat16, shape=(512, 160)), None, True, supported=sup) is False
    assert ok("all", lp, x, None, idx, 2, nn_, fc2, NS(dtype=F32, shape=(512, 80)), None, True, supported=sup) is False
    monkeypatch.setattr(fused, "MR_GEMM", False)
    assert ok("all", lp, x, None, idx, 2, nn_, fc2, res, None, True, supported=sup) is False            # MR_GEMM off
    monkeypatch.setattr(fused, "MR_GEMM", True)
    assert ok("all", lp, x, None, idx, 2, nn_, fc2, res, None, True, supported=lambda *a: False) is False      # the library says no
    # ... and the rest of the list
    assert ok("all", lp, NS(dtype=torch.bfloat16, shape=(2, 256, 160)), None, idx, 2, nn_, fc2, res, None, True, supported=sup) is False
    assert ok("all", lp, x, None, NS(dtype=torch.int16, shape=(4, 255, 9)), 2, nn_, fc2, res, None, True, supported=sup) is False
    assert ok("all", lp, x, None, idx, 2, nn_, _layer(160, 160), res, None, True, supported=sup) is False      # fc2 does not contract 2C
    assert ok("all", lp, x, None, idx, 8, nn_, fc2, res, None, True, supported=sup) is False            # lists of another grouping
    xw = NS(dtype=F32, shape=(2, 36, 640))                                                              # beyond the envelope: the library says no
    assert ok("all", lp, xw, None, NS(dtype=torch.int16, shape=(4, 36, 9)), 2, _layer(1280, 1280, groups=4) + (object(),),
              _layer(1280, 640), None, None, True) is False
    # the measured rule stands between the plain switch and the library; "all" bypasses it
    from gkgnet_amd import linear_bf16
    monkeypatch.setattr(linear_bf16, "mr_fc2_pays", lambda T, C: False)
    assert ok(True, lp, x, None, idx, 2, nn_, fc2, res, None, True, supported=sup) is False
    assert ok("all", lp, x, None, idx, 2, nn_, fc2, res, None, True, supported=sup) is True
    monkeypatch.setattr(linear_bf16, "mr_fc2_pays", lambda T, C: True)
    assert ok(True, lp, x, None, idx, 2, nn_, fc2, res, None, True, supported=sup) is True
