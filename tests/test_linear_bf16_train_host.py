"""GKG_ENABLE=train_bf16 (gkg_linear_bf16_f32a, gkg_linear_wgrad_bf16; linear_bf16.py), the parts that need no device: the ABI
version and the four entry points in the derived binding, the pure host functions, the dispatch predicate and the fragment
array of the transposed weight."""
import ctypes as C
import functools
import types

import torch

I, P = C.c_int, C.c_void_p
NEW = ("gkg_linear_bf16_f32a", "gkg_linear_bf16_f32a_supported", "gkg_linear_wgrad_bf16", "gkg_linear_wgrad_bf16_supported")


def test_abi_16_binds_the_four_entry_points():
    from gkgnet_amd import _abi, _lib
    assert _lib.ABI_VERSION >= 16
    protos = _abi.header().protos
    for name in NEW:
        assert name in protos and name in _lib.EXPORTS, name
    assert protos["gkg_linear_bf16_f32a"] == protos["gkg_linear_bf16"]          # the same argument list (x is a pointer either way)
    assert protos["gkg_linear_bf16_f32a_supported"] == (I, [I] * 7)
    assert protos["gkg_linear_wgrad_bf16"] == (I, [P, I, P, I, P, I, I, I, P])
    assert protos["gkg_linear_wgrad_bf16_supported"] == (I, [I] * 3)
    lib = _lib.load()
    assert lib.gkg_version() == _lib.ABI_VERSION
    for name in NEW:
        assert hasattr(lib, name)


def test_host_functions_answer_without_a_device():
    from gkgnet_amd import _abi, _lib
    lib = _lib.load()
    for R, cin, cout in [(1, 16, 8), (324, 80, 80), (65, 2560, 640), (16400, 80, 1280)]:
        assert lib.gkg_linear_bf16_f32a_supported(R, cin, cout, 1, 1, 0, 0) == 1
        assert lib.gkg_linear_wgrad_bf16_supported(R, cin, cout) == 1
    for R, cin, cout in [(65, 12, 80), (65, 80, 20), (0, 80, 80)]:
        assert lib.gkg_linear_bf16_f32a_supported(R, cin, cout, 0, 1, 0, 0) == 0
        assert lib.gkg_linear_wgrad_bf16_supported(R, cin, cout) == 0
    assert lib.gkg_linear_bf16_f32a_supported(65, 80, 80, 0, 0, 0, 0) == 0       # no output wanted
    # the slab length is R rounded up to a 32-row chunk and must fit an int
    assert lib.gkg_linear_wgrad_bf16_supported(2 ** 31 - 1, 80, 80) == 0
    assert lib.gkg_linear_wgrad_bf16_supported(2 ** 31 - 1 - 32, 80, 80) == 1
    # null pointers and bad sizes come back as codes with nothing launched (no device is touched before the checks)
    err_null = _abi.header().constants["ERR_NULL"]
    assert lib.gkg_linear_wgrad_bf16(None, 80, None, 80, None, 65, 80, 80, None) == err_null
    assert lib.gkg_linear_bf16_f32a(None, 80, None, None, None, None, 0, None, 80, None, 0, 65, 80, 80, 0, None) == err_null


def test_switch_is_off_by_default():
    import os
    from gkgnet_amd import fused
    if "train_bf16" not in os.environ.get("GKG_ENABLE", ""):
        assert fused.TRAIN_BF16 is False


def _x(dtype=torch.float32, shape=(324, 80), strides=(80, 1), cuda=True):
    return types.SimpleNamespace(dtype=dtype, shape=shape, is_cuda=cuda, stride=lambda d: strides[d])


def _conv(groups=1, wshape=(160, 80, 1, 1)):
    return types.SimpleNamespace(groups=groups, weight=types.SimpleNamespace(shape=wshape))


def test_train_predicate_truth_table(monkeypatch):
    """Every condition fails alone.  Plain Python objects: no CUDA tensor, no autocast context (the two torch queries are answered
    by the test)."""
    from gkgnet_amd import fused
    auto = {"on": True, "dtype": torch.bfloat16}
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: auto["on"])
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: auto["dtype"])
    monkeypatch.setattr(fused, "DETERMINISTIC", False)
    sup = lambda R, cin, cout: (R, cin, cout) == (324, 80, 160)                   # noqa: E731
    ok = functools.partial(fused.train16_ok, fused.BF16)
    bn = types.SimpleNamespace(training=True, track_running_stats=True)
    x, conv = _x(), _conv()
    with torch.enable_grad():
        assert ok(True, x, conv, bn, supported=sup) is True
        assert ok(True, x, conv, bn) is True                                     # the library's own three answers (host code)
        assert ok(False, x, conv, bn, supported=sup) is False                    # switch off
        with torch.no_grad():
            assert ok(True, x, conv, bn, supported=sup) is False                 # no gradients
        auto["on"] = False
        assert ok(True, x, conv, bn, supported=sup) is False                     # no autocast
        auto["on"] = True
        auto["dtype"] = torch.float16
        assert ok(True, x, conv, bn, supported=sup) is False                     # fp16 autocast
        auto["dtype"] = torch.bfloat16
        monkeypatch.setattr(fused, "DETERMINISTIC", True)
        assert ok(True, x, conv, bn, supported=sup) is False                     # GKG_DETERMINISTIC
        monkeypatch.setattr(fused, "DETERMINISTIC", False)
        assert ok(True, _x(dtype=torch.bfloat16), conv, bn, supported=sup) is False             # bf16 x
        assert ok(True, _x(cuda=False), conv, bn, supported=sup) is False                       # a CPU tensor
        assert ok(True, _x(shape=(2, 162, 80), strides=(12960, 80, 1)), conv, bn, supported=sup) is False
        assert ok(True, _x(strides=(1, 324)), conv, bn, supported=sup) is False                 # column stride
        assert ok(True, _x(strides=(82, 1)), conv, bn, supported=sup) is False                  # pitch % 4
        assert ok(True, _x(strides=(84, 1)), conv, bn, supported=sup) is True                   # a pitched matrix is fine
        assert ok(True, x, _conv(groups=4, wshape=(160, 20, 1, 1)), bn, supported=sup) is False   # grouped conv
        assert ok(True, x, _conv(groups=4), bn, supported=sup) is False
        assert ok(True, x, _conv(wshape=(160, 80, 3, 3)), bn, supported=sup) is False             # 3x3 weight
        assert ok(True, x, _conv(wshape=(160, 96, 1, 1)), bn, supported=sup) is False             # cin mismatch
        assert ok(True, x, conv, bn, supported=lambda *a: False) is False                       # the library says no
        assert ok(True, _x(shape=(324, 12), strides=(12, 1)), _conv(wshape=(160, 12, 1, 1)), bn) is False      # ... itself: cin % 8
        assert ok(True, x, conv, bn, supported=sup) is True                      # (and the table's state is back where it began)


def _fragments(w2d):
    """The test's own statement of the fragment layout (include/gkg_hip.h) for a (columns, contraction) matrix: [k_pad / 8][n_pad][8]
    with fragment (f, n) = w2d[n][8f .. 8f+7], contraction padded to 16, columns to 32."""
    n, k = w2d.shape
    n_pad, k_pad = (n + 31) // 32 * 32, (k + 15) // 16 * 16
    p = torch.zeros(k_pad // 8, n_pad, 8, dtype=torch.bfloat16)
    w16 = w2d.to(torch.bfloat16)
    for f in range((k + 7) // 8):
        for j in range(n):
            p[f, j, :min(8, k - 8 * f)] = w16[j, 8 * f:8 * f + 8]
    return p


def test_transposed_planes_are_the_fragments_of_w_t_and_cached():
    from gkgnet_amd import _lib, derived
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(24, 40, 1)                                            # cout 40 -> contraction pad 48, cin 24 -> 32 columns
    pt = derived.lin_planes(conv, transposed=True)
    assert pt.dtype == torch.bfloat16 and pt.is_contiguous() and tuple(pt.shape) == (6, 32, 8)
    assert pt.numel() * 2 == _lib.load().gkg_linear_bf16_planes_bytes(40, 24)
    w = conv.weight.detach().reshape(40, 24)
    assert torch.equal(pt.view(torch.int16), _fragments(w.t()).view(torch.int16))
    # the forward array is the same layout of w itself: the two are one construction
    assert torch.equal(derived.lin_planes(conv).view(torch.int16), _fragments(w).view(torch.int16))
    assert bool((pt[5] == 0).all()) and bool((pt[:, 24:] == 0).all())            # the pad region
    assert derived.lin_planes(conv, transposed=True) is pt                                    # cached
    with torch.no_grad():
        conv.weight.mul_(2.0)                                                    # an in-place parameter update
    pt2 = derived.lin_planes(conv, transposed=True)
    assert pt2 is not pt and torch.equal(pt2.float(), 2.0 * pt.float())
    assert torch.equal(pt2.view(torch.int16), _fragments(conv.weight.detach().reshape(40, 24).t()).view(torch.int16))
