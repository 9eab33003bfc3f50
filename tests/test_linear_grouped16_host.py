"""GKG_ENABLE=train_grouped, the parts that need no device: the four grouped prototypes in the header and the derived binding, the
envelope of ``*_grouped_supported`` (pure host code), the stacked fragment arrays of the grouped weight (derived.glin_planes), the
new fields of the kind table and the predicate / decision that walk it (linear_bf16.train16_grouped_ok,
fused._train_grouped_16bit).  Reference layer: BasicConv's Conv2d(1x1, groups = 4) (torch_nn.py:57-69 behind torch_vertex.py:57-61)."""
import os
import re
import types

import pytest
import torch

NAMES = ("gkg_linear_bf16_f32a_grouped", "gkg_linear_bf16_f32a_grouped_supported",
         "gkg_linear_f16_f32a_grouped", "gkg_linear_f16_f32a_grouped_supported")


def test_header_declares_the_four_prototypes():
    from gkgnet_amd import _abi, _lib
    protos = _abi.header().protos
    for name in NAMES:
        assert name in protos and name in _lib.EXPORTS, name
    assert protos["gkg_linear_f16_f32a_grouped"] == protos["gkg_linear_bf16_f32a_grouped"]
    assert protos["gkg_linear_f16_f32a_grouped_supported"] == protos["gkg_linear_bf16_f32a_grouped_supported"]
    text = open(os.path.join(os.path.dirname(_lib.PKG), "include", "gkg_hip.h")).read()
    m = re.search(r"#define GKG_ABI_VERSION (\d+)", text)
    assert m and int(m.group(1)) == _lib.ABI_VERSION >= 22
    assert _lib.load().gkg_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("fn", [NAMES[1], NAMES[3]])
def test_supported_envelope(fn):
    from gkgnet_amd import _lib
    sup = getattr(_lib.load(), fn)
    for ok in ((1, 8, 8, 1), (162, 24, 24, 4), (10368, 320, 320, 4), (129, 24, 24, 64)):
        assert sup(*ok) == 1, ok
    for bad in ((162, 12, 24, 4), (162, 24, 20, 4), (162, 24, 24, 0), (162, 24, 24, 65), (0, 24, 24, 4), (162, 0, 24, 4),
                (162, 24, 0, 4), (162, 24, 24, -1)):
        assert sup(*bad) == 0, bad
    # nb x tiles <= 0x3fffffff: 2^31 - 1 rows are 2^24 row tiles of one column tile
    assert sup(0x7FFFFFFF, 8, 8, 63) == 1 and sup(0x7FFFFFFF, 8, 8, 64) == 0
    assert sup(0x7FFFFFFF, 8, 72, 31) == 1 and sup(0x7FFFFFFF, 8, 72, 32) == 0


def _frag_bytes(lib, kind, n, k):
    return int(getattr(lib, kind.planes_bytes)(k, n))


@pytest.mark.parametrize("cin_cout", [(48, 96), (96, 96)], ids=str)
def test_glin_planes_are_the_fragments_of_the_permuted_groups(cin_cout):
    """Group by group the array equals derived._fragments of _kperm_weight(Wg)[q] (forward) or of its transpose (input gradient), in
    the kind's dtype, cached in the kind's grouped slot, rebuilt after an in-place update; the four dense slots stay empty."""
    from gkgnet_amd import _lib, derived, fused, linear_bf16
    cin, cout = cin_cout
    conv = torch.nn.Conv2d(cin, cout, 1, groups=4)
    nb, co, ci = 4, cout // 4, cin // 4
    for kind in linear_bf16.KINDS.values():
        for transposed in (False, True):
            slot = kind.gslots[transposed]
            assert derived.peek(conv, slot) is None
            p = derived.glin_planes(conv, kind, transposed)
            assert p.dtype == kind.fragment and p.shape[0] == nb and p.is_contiguous()
            assert derived.peek(conv, slot) is p and derived.glin_planes(conv, kind.name, transposed=transposed) is p
            Wp = fused._kperm_weight(conv.weight.detach().view(nb, co, ci))
            n, k = (ci, co) if transposed else (co, ci)
            for q in range(nb):
                m = Wp[q].t() if transposed else Wp[q]
                want = derived._fragments(m, derived._up(k, derived.K_ALIGN), derived._up(n, derived.N_ALIGN), kind.fragment)
                assert torch.equal(p[q], want), (kind.name, transposed, q)
            if ci % 8 == 0 and co % 8 == 0:                                      # a shape the kernels take: the library's own size
                assert p.numel() * 2 == nb * _frag_bytes(_lib.load(), kind, n, k)
                assert p[0].numel() * 2 == _frag_bytes(_lib.load(), kind, n, k)
    with torch.no_grad():
        conv.weight.add_(0.25)
    for kind in linear_bf16.KINDS.values():
        for transposed in (False, True):
            old = derived.peek(conv, kind.gslots[transposed])
            new = derived.glin_planes(conv, kind, transposed)
            assert new is not old and not torch.equal(new, old)
            assert derived.peek(conv, kind.gslots[transposed]) is new
        for slot in kind.slots:
            assert derived.peek(conv, slot) is None


def test_the_kind_rows_gain_the_grouped_fields_and_keep_the_old_ones():
    from gkgnet_amd import linear_bf16
    B, F = linear_bf16.BF16, linear_bf16.F16
    assert (B.f32a_grouped, B.f32a_grouped_supported) == NAMES[:2] and (F.f32a_grouped, F.f32a_grouped_supported) == NAMES[2:]
    assert B.gslots == ("glin_planes", "glin_planes_t") and F.gslots == ("glin_planes_f16", "glin_planes_t_f16")
    every = [s for k in (B, F) for s in k.slots + k.gslots]
    assert len(set(every)) == 8
    assert tuple(B)[:8] == ("bf16", torch.bfloat16, "gkg_linear_bf16_f32a", "gkg_linear_bf16_f32a_supported",
                            "gkg_linear_bf16_planes_bytes", torch.bfloat16, ("lin_planes", "lin_planes_t"), True)
    assert tuple(F)[:8] == ("f16", torch.float16, "gkg_linear_f16_f32a", "gkg_linear_f16_f32a_supported",
                            "gkg_linear_f16_planes_bytes", torch.float16, ("lin_planes_f16", "lin_planes_t_f16"), False)
    assert linear_bf16.Kind16._fields[:8] == ("name", "autocast", "f32a", "f32a_supported", "planes_bytes", "fragment", "slots",
                                              "own_wgrad")


def _xm(R=162, cols=96, col_stride=1):
    return types.SimpleNamespace(dtype=torch.float32, shape=(R, cols), is_cuda=True, stride=lambda d: (cols * col_stride, col_stride)[d])


def _conv(groups=4, wshape=(96, 24, 1, 1)):
    return types.SimpleNamespace(groups=groups, weight=types.SimpleNamespace(shape=wshape))


def test_the_predicate_and_the_decision(monkeypatch):
    """Plain Python objects: no CUDA tensor, no autocast context (the two torch queries are answered by the test)."""
    from gkgnet_amd import fused, linear_bf16
    auto = {"dtype": torch.bfloat16, "on": True}
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: auto["on"])
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: auto["dtype"])
    monkeypatch.setattr(fused, "DETERMINISTIC", False)
    bn = types.SimpleNamespace(training=True, track_running_stats=True)
    asked = []

    def yes(R, cin, cout, nb):
        asked.append((R, cin, cout, nb))
        return True
    rows = ((torch.bfloat16, "TRAIN_BF16", linear_bf16.BF16), (torch.float16, "TRAIN_F16", linear_bf16.F16))
    ok = linear_bf16.train16_grouped_ok
    with torch.enable_grad():
        for dtype, _, kind in rows:
            auto["dtype"] = dtype
            asked.clear()
            assert ok(kind, True, _xm(), _conv(), bn, supported=yes)
            assert asked == [(162, 24, 24, 4), (162, 24, 24, 4)]                  # forward, then the input gradient's transposed sizes
            assert not ok(kind, False, _xm(), _conv(), bn, supported=yes)
            assert not ok(kind, True, _xm(), _conv(), bn, supported=lambda *a: False)
            assert not ok(kind, True, _xm(), _conv(groups=1), bn, supported=yes)                  # groups != 4
            assert not ok(kind, True, _xm(), _conv(groups=2), bn, supported=yes)
            assert not ok(kind, True, _xm(), _conv(wshape=(96, 48, 1, 1)), bn, supported=yes)     # not over exactly XM's columns
            assert not ok(kind, True, _xm(), _conv(wshape=(96, 24, 3, 3)), bn, supported=yes)     # not 1x1
            assert not ok(kind, True, _xm(), _conv(wshape=(96, 24)), bn, supported=yes)
            assert not ok(kind, True, _xm(col_stride=2), _conv(), bn, supported=yes)              # a non-unit column stride
            x16 = _xm()
            x16.dtype = dtype
            assert not ok(kind, True, x16, _conv(), bn, supported=yes)                            # XM itself must be fp32
            auto["dtype"] = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16          # the other kind's autocast dtype
            assert not ok(kind, True, _xm(), _conv(), bn, supported=yes)
            auto["dtype"] = dtype
            auto["on"] = False
            assert not ok(kind, True, _xm(), _conv(), bn, supported=yes)
            auto["on"] = True
            with torch.no_grad():
                assert not ok(kind, True, _xm(), _conv(), bn, supported=yes)                      # gradients off
            asked.clear()
            assert ok(kind, True, _xm(cols=64), _conv(wshape=(160, 16, 1, 1)), bn, supported=yes)  # ci != co: both orientations asked
            assert asked == [(162, 16, 40, 4), (162, 40, 16, 4)]
        # the decision: the library's own answer (pure host code), the switches' conjunction, the kind by the autocast dtype
        conv = _conv()
        for dtype, switch, kind in rows:
            auto["dtype"] = dtype
            for det in (False, True):                                            # GKG_DETERMINISTIC does not refuse, for either kind
                monkeypatch.setattr(fused, "DETERMINISTIC", det)
                monkeypatch.setattr(fused, "TRAIN_BF16", True)
                monkeypatch.setattr(fused, "TRAIN_F16", True)
                monkeypatch.setattr(fused, "TRAIN_GROUPED", True)
                got = fused._train_grouped_16bit(_xm(), conv, bn)
                assert got is not None and got[0] is kind and got[1] is conv
                monkeypatch.setattr(fused, "TRAIN_GROUPED", False)
                assert fused._train_grouped_16bit(_xm(), conv, bn) is None
                monkeypatch.setattr(fused, "TRAIN_GROUPED", True)
                monkeypatch.setattr(fused, switch, False)                        # the kind's own switch off, the other's on
                assert fused._train_grouped_16bit(_xm(), conv, bn) is None
            monkeypatch.setattr(fused, switch, True)
            assert fused._train_grouped_16bit(_xm(cols=48), _conv(wshape=(96, 12, 1, 1)), bn) is None      # ci % 8: the library refuses
