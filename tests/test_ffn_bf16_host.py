"""gkg_ffn_bf16 (csrc/gkg_ffn_bf16.hip), the parts that need no device: the two entry points in the header and the derived binding,
the pure host predicate, the opt-in switch and the dispatch predicate of ``fused.ffn_forward``."""
import ctypes as C
import types

import torch

I, P, F = C.c_int, C.c_void_p, C.c_void_p


def test_header_declares_the_two_entry_points():
    from gkgnet_amd import _abi, _lib
    assert _lib.ABI_VERSION >= 17
    protos = _abi.header().protos
    assert protos["gkg_ffn_bf16_supported"] == (I, [I] * 8)
    assert protos["gkg_ffn_bf16"] == (I, [P, I, P, F, F, P, F, F, F, I, F, I, P, I, I, I, I, I, I, P])
    for name in ("gkg_ffn_bf16_supported", "gkg_ffn_bf16"):
        assert name in _lib.EXPORTS
    lib = _lib.load()
    assert lib.gkg_version() == _lib.ABI_VERSION


def test_host_predicate_answers_without_a_device():
    from gkgnet_amd import _lib
    lib = _lib.load()
    # the envelope: multiples of 8, cin <= 192, cout <= 192, any hid, any R >= 1, cin != cout allowed
    for R, cin, hid, cout in [(1, 16, 8, 16), (663552, 80, 320, 80), (589824, 96, 384, 96), (165888, 160, 640, 160),
                              (147456, 192, 768, 192), (65, 96, 200, 80), (65, 192, 4096, 8), (65, 8, 72, 192)]:
        for has_res, w32, w16, act in [(0, 1, 0, 0), (1, 1, 1, 1), (0, 0, 1, 1), (1, 1, 0, 0)]:
            assert lib.gkg_ffn_bf16_supported(R, cin, hid, cout, has_res, w32, w16, act) == 1, (R, cin, hid, cout)
    for R, cin, hid, cout in [(65, 12, 80, 80), (65, 80, 20, 80), (65, 80, 80, 20), (0, 80, 320, 80)]:
        assert lib.gkg_ffn_bf16_supported(R, cin, hid, cout, 1, 1, 1, 1) == 0
    assert lib.gkg_ffn_bf16_supported(65, 80, 320, 80, 1, 0, 0, 1) == 0          # no output wanted
    assert lib.gkg_ffn_bf16_supported(65, 80, 320, 80, 1, 1, 1, 2) == 0          # unknown activation


def test_switch_is_off_by_default_and_documented():
    import os
    from gkgnet_amd import fused
    if "ffn_bf16" not in os.environ.get("GKG_ENABLE", ""):
        assert fused.FFN_BF16 is False
    assert "ffn_bf16" in open(fused.__file__).read().split("_DISABLED = _env_list")[0]      # the GKG_ENABLE comment table


def _layer(cin, cout, training=False, groups=1):
    conv = types.SimpleNamespace(groups=groups, weight=types.SimpleNamespace(shape=(cout, cin // groups, 1, 1)))
    return (conv, types.SimpleNamespace(training=training, track_running_stats=True))


def test_dispatch_predicate_truth_table(monkeypatch):
    """One flipped input per row turns the dispatch off.  Plain Python objects: no CUDA tensor, no autocast context (the two torch
    queries lowp_inference reads are answered by the test)."""
    from gkgnet_amd import fused
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.bfloat16)
    asked = []

    def sup(R, cin, hid, cout):
        asked.append((R, cin, hid, cout))
        return (R, cin, hid, cout) == (324, 160, 640, 160)
    ok = fused.ffn_bf16_ok
    with torch.no_grad():
        lp = fused.lowp_inference()
    assert lp is True
    x = types.SimpleNamespace(dtype=torch.bfloat16, shape=(324, 160))
    res = types.SimpleNamespace(dtype=torch.float32, shape=(324, 160))
    fc1, fc2 = _layer(160, 640), _layer(640, 160)
    assert ok(True, lp, x, fc1, fc2, res, None, True, supported=sup) is True
    assert asked == [(324, 160, 640, 160)]
    assert ok(True, lp, x, fc1, fc2, None, None, True, supported=sup) is True                  # no residual
    assert ok(True, lp, x, fc1, fc2, res, None, True) is True                                  # the library's own answer (host code)
    assert ok(False, lp, x, fc1, fc2, res, None, True, supported=sup) is False                 # switch off
    with torch.enable_grad():
        assert ok(True, fused.lowp_inference(), x, fc1, fc2, res, None, True, supported=sup) is False      # not lowp_inference
    assert ok(True, lp, x, fc1, fc2, res, None, False, supported=sup) is False                 # off the channels-last chain
    assert ok(True, lp, x, _layer(160, 640, training=True), fc2, res, None, True, supported=sup) is False   # a train-mode BN
    assert ok(True, lp, x, fc1, _layer(640, 160, training=True), res, None, True, supported=sup) is False
    assert ok(True, lp, x, _layer(160, 640, groups=4), fc2, res, None, True, supported=sup) is False        # a grouped conv
    assert ok(True, lp, x, fc1, _layer(640, 160, groups=4), res, None, True, supported=sup) is False
    assert ok(True, lp, x, fc1, fc2, res, object(), True, supported=sup) is False              # a DropPath scale
    # ... and the rest of the list
    assert ok(True, lp, x, fc1, fc2, res, None, True, supported=sup, act=0) is False           # the hidden's activation is not GELU
    assert ok(True, lp, types.SimpleNamespace(dtype=torch.float32, shape=(324, 160)), fc1, fc2, res, None, True, supported=sup) is False
    assert ok(True, lp, x, fc1, _layer(320, 160), res, None, True, supported=sup) is False     # fc2 does not contract the hidden
    assert ok(True, lp, x, fc1, fc2, types.SimpleNamespace(dtype=torch.float32, shape=(324, 80)), None, True, supported=sup) is False
    assert ok(True, lp, x, fc1, fc2, types.SimpleNamespace(dtype=torch.bfloat16, shape=(324, 160)), None, True, supported=sup) is False
    assert ok(True, lp, x, fc1, fc2, res, None, True, supported=lambda *a: False) is False
    xw = types.SimpleNamespace(dtype=torch.bfloat16, shape=(36, 640))                          # beyond the envelope: the library says no
    assert ok(True, lp, xw, _layer(640, 2560), _layer(2560, 640), None, None, True) is False
