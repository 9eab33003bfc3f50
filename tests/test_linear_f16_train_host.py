"""GKG_ENABLE=train_f16 (gkg_linear_f16_f32a; linear_bf16.py, derived.py), the parts that need no device: the ABI version and the
three entry points in the derived binding, the pure host functions, the fp16 fragment layout and the dispatch predicate."""
import ctypes as C
import functools
import itertools
import re
import types

import torch

I = C.c_int
NEW = ("gkg_linear_f16_planes_bytes", "gkg_linear_f16_f32a_supported", "gkg_linear_f16_f32a")


def test_abi_21_declares_binds_and_exports_the_three_symbols():
    from gkgnet_amd import _abi, _build, _lib
    with open(_build.INCLUDE + "/gkg_hip.h") as fh:
        text = fh.read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
    m = re.search(r"#define GKG_ABI_VERSION (\d+)", text)
    assert m and int(m.group(1)) == _lib.ABI_VERSION >= 21
    protos = _abi.header().protos
    for name in NEW:
        assert name in protos and name in _lib.EXPORTS, name
    assert protos["gkg_linear_f16_f32a"] == protos["gkg_linear_bf16_f32a"]       # the same argument list
    assert protos["gkg_linear_f16_f32a_supported"] == (I, [I] * 7)
    assert protos["gkg_linear_f16_planes_bytes"] == (C.c_size_t, [I, I])
    lib = _lib.load()
    assert lib.gkg_version() == _lib.ABI_VERSION
    for name in NEW:
        assert hasattr(lib, name)


def test_planes_bytes_are_the_bf16_paddings():
    from gkgnet_amd import _lib
    lib = _lib.load()
    for cin, cout in [(16, 8), (40, 72), (400, 1600)]:
        assert lib.gkg_linear_f16_planes_bytes(cin, cout) == lib.gkg_linear_bf16_planes_bytes(cin, cout) > 0
    assert lib.gkg_linear_f16_planes_bytes(40, 72) == (48 // 8) * 96 * 16
    for cin, cout in [(12, 80), (80, 20), (0, 80), (80, 0), (-8, 8)]:
        assert lib.gkg_linear_f16_planes_bytes(cin, cout) == 0


def test_supported_agrees_with_the_bf16_entry_point():
    from gkgnet_amd import _abi, _lib
    lib = _lib.load()
    seen = set()
    for R, cin, cout, res, w32, w16, act in itertools.product((0, 1, 324, 16400, 2 ** 31 - 1), (8, 12, 80), (8, 20, 1600), (0, 1),
                                                              (0, 1), (0, 1), (0, 1, 2)):
        got = lib.gkg_linear_f16_f32a_supported(R, cin, cout, res, w32, w16, act)
        assert got == lib.gkg_linear_bf16_f32a_supported(R, cin, cout, res, w32, w16, act), (R, cin, cout, res, w32, w16, act)
        seen.add(got)
    assert seen == {0, 1}
    # null pointers come back as a code with nothing launched (no device is touched before the checks)
    err_null = _abi.header().constants["ERR_NULL"]
    assert lib.gkg_linear_f16_f32a(None, 80, None, None, None, None, 0, None, 80, None, 0, 65, 80, 80, 0, None) == err_null
    assert b"gkg_linear_f16_f32a" in lib.gkg_last_error_string()


def test_switch_is_off_by_default():
    import os
    from gkgnet_amd import fused
    if "train_f16" not in os.environ.get("GKG_ENABLE", ""):
        assert fused.TRAIN_F16 is False


def _fragments(w2d):
    """The test's own statement of the layout (include/gkg_hip.h) for a (columns n, contraction k) matrix: [k_pad / 8][n_pad][8] with
    fragment (f, n) = w2d[n][8f .. 8f+7], zero outside; contraction padded to 16, columns to 32."""
    n, k = w2d.shape
    n_pad, k_pad = (n + 31) // 32 * 32, (k + 15) // 16 * 16
    p = torch.zeros(k_pad // 8, n_pad, 8, dtype=torch.float16)
    w16 = w2d.to(torch.float16)
    for f in range((k + 7) // 8):
        for j in range(n):
            p[f, j, :min(8, k - 8 * f)] = w16[j, 8 * f:8 * f + 8]
    return p


def test_f16_fragments_against_an_explicit_loop():
    from gkgnet_amd import derived
    for n, k in [(5, 12), (33, 40)]:
        g = torch.Generator().manual_seed(100 * n + k)
        w = torch.randn(n, k, generator=g)
        w[0, 0], w[n - 1, k - 1] = 1.0e5, 3.0e-6                                 # beyond fp16's range (-> inf) and an fp16 subnormal
        n_pad, k_pad = (n + 31) // 32 * 32, (k + 15) // 16 * 16
        p = derived.f16_fragments(w, k_pad, n_pad)
        assert p.dtype == torch.float16 and p.is_contiguous() and tuple(p.shape) == (k_pad // 8, n_pad, 8)
        assert torch.equal(p.view(torch.int16), _fragments(w).view(torch.int16))
        assert bool(torch.isinf(p[0, 0, 0])) and float(p[(k - 1) // 8, n - 1, (k - 1) % 8]) != 0.0
        assert bool((p[:, n:] == 0).all())


def test_f16_plane_slots_are_cached_and_follow_updates():
    from gkgnet_amd import _lib, derived
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(24, 40, 1)
    p, pt = derived.lin_planes(conv, "f16"), derived.lin_planes(conv, "f16", transposed=True)
    assert p.dtype == pt.dtype == torch.float16 and tuple(p.shape) == (4, 64, 8) and tuple(pt.shape) == (6, 32, 8)
    lib = _lib.load()
    assert p.numel() * 2 == lib.gkg_linear_f16_planes_bytes(24, 40) and pt.numel() * 2 == lib.gkg_linear_f16_planes_bytes(40, 24)
    w = conv.weight.detach().reshape(40, 24)
    assert torch.equal(p.view(torch.int16), _fragments(w).view(torch.int16))
    assert torch.equal(pt.view(torch.int16), _fragments(w.t()).view(torch.int16))
    assert derived.lin_planes(conv, "f16") is p and derived.lin_planes(conv, "f16", transposed=True) is pt
    assert derived.lin_planes(conv).dtype == torch.bfloat16                      # the bf16 slots are their own
    with torch.no_grad():
        conv.weight.mul_(2.0)
    p2, pt2 = derived.lin_planes(conv, "f16"), derived.lin_planes(conv, "f16", transposed=True)
    assert p2 is not p and pt2 is not pt
    w2 = conv.weight.detach().reshape(40, 24)
    assert not torch.equal(p2, p) and not torch.equal(pt2, pt)
    assert torch.equal(p2.view(torch.int16), _fragments(w2).view(torch.int16))
    assert torch.equal(pt2.view(torch.int16), _fragments(w2.t()).view(torch.int16))


def _x(dtype=torch.float32, shape=(324, 80), strides=(80, 1), cuda=True):
    return types.SimpleNamespace(dtype=dtype, shape=shape, is_cuda=cuda, stride=lambda d: strides[d])


def _conv(groups=1, wshape=(160, 80, 1, 1)):
    return types.SimpleNamespace(groups=groups, weight=types.SimpleNamespace(shape=wshape))


def test_train_f16_predicate_truth_table(monkeypatch):
    """Plain Python objects: no CUDA tensor, no autocast context (the two torch queries are answered by the test)."""
    from gkgnet_amd import fused
    auto = {"on": True, "dtype": torch.float16}
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: auto["on"])
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: auto["dtype"])
    monkeypatch.setattr(fused, "DETERMINISTIC", False)
    sup = lambda R, cin, cout: (R, cin, cout) == (324, 80, 160)                   # noqa: E731
    ok = functools.partial(fused.train16_ok, fused.F16)
    bn = types.SimpleNamespace(training=True, track_running_stats=True)
    x, conv = _x(), _conv()
    with torch.enable_grad():
        assert ok(True, x, conv, bn, supported=sup) is True
        assert ok(True, x, conv, bn) is True                                     # the library's own two answers (host code)
        assert ok(False, x, conv, bn, supported=sup) is False                    # switch off
        auto["dtype"] = torch.bfloat16
        assert ok(True, x, conv, bn, supported=sup) is False                     # bf16 autocast
        auto["dtype"] = torch.float16
        auto["on"] = False
        assert ok(True, x, conv, bn, supported=sup) is False                     # no autocast
        auto["on"] = True
        with torch.no_grad():
            assert ok(True, x, conv, bn, supported=sup) is False                 # no gradients
        assert ok(True, x, _conv(groups=4, wshape=(160, 20, 1, 1)), bn, supported=sup) is False   # grouped conv
        assert ok(True, x, _conv(groups=4), bn, supported=sup) is False
        assert ok(True, _x(strides=(82, 1)), conv, bn, supported=sup) is False                  # pitch % 4
        assert ok(True, _x(strides=(84, 1)), conv, bn, supported=sup) is True                   # a pitched matrix is fine
        assert ok(True, _x(dtype=torch.float16), conv, bn, supported=sup) is False              # fp16 x
        assert ok(True, _x(cuda=False), conv, bn, supported=sup) is False
        assert ok(True, _x(strides=(1, 324)), conv, bn, supported=sup) is False                 # column stride
        assert ok(True, _x(shape=(2, 162, 80), strides=(12960, 80, 1)), conv, bn, supported=sup) is False
        assert ok(True, x, _conv(wshape=(160, 80, 3, 3)), bn, supported=sup) is False
        assert ok(True, x, _conv(wshape=(160, 96, 1, 1)), bn, supported=sup) is False             # cin mismatch
        assert ok(True, x, conv, bn, supported=lambda *a: False) is False                       # the library says no
        assert ok(True, _x(shape=(324, 12), strides=(12, 1)), _conv(wshape=(160, 12, 1, 1)), bn) is False      # ... itself: cin % 8
        monkeypatch.setattr(fused, "DETERMINISTIC", True)
        assert ok(True, x, conv, bn, supported=sup) is True                      # GKG_DETERMINISTIC does not exclude it
        assert ok(True, x, conv, bn) is True


def test_the_two_switches_do_not_see_each_other(monkeypatch):
    """train16_ok's bf16 answers are what they were, whatever TRAIN_F16 is; the one decision of ``fused`` returns the kind that
    belongs to the autocast dtype, with both switches on too."""
    from gkgnet_amd import fused
    auto = {"on": True, "dtype": torch.bfloat16}
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: auto["on"])
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: auto["dtype"])
    monkeypatch.setattr(fused, "DETERMINISTIC", False)
    bn = types.SimpleNamespace(training=True, track_running_stats=True)
    x, conv = _x(), _conv()
    bf16_ok = functools.partial(fused.train16_ok, fused.BF16)
    with torch.enable_grad():
        for f16 in (False, True):
            monkeypatch.setattr(fused, "TRAIN_F16", f16)
            auto["dtype"] = torch.bfloat16
            assert bf16_ok(True, x, conv, bn) is True and bf16_ok(False, x, conv, bn) is False
            auto["dtype"] = torch.float16
            assert bf16_ok(True, x, conv, bn) is False
        want = {(False, False): (None, None), (True, False): ("bf16", None), (False, True): (None, "f16"), (True, True): ("bf16", "f16")}
        for (b16, f16), (under_bf16, under_f16) in want.items():
            monkeypatch.setattr(fused, "TRAIN_BF16", b16)
            monkeypatch.setattr(fused, "TRAIN_F16", f16)
            for dtype, kind in ((torch.bfloat16, under_bf16), (torch.float16, under_f16)):
                auto["dtype"] = dtype
                got = fused._train_16bit(x, conv, bn)
                assert (got is None and kind is None) or (got[0].name == kind and got[1] is conv), (b16, f16, dtype, got)
            auto["on"] = False
            assert fused._train_16bit(x, conv, bn) is None                       # fp32
            auto["on"] = True
