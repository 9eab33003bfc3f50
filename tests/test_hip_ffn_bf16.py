"""gkg_ffn_bf16 (csrc/gkg_ffn_bf16.hip): an FFN's two bf16 projections (fc1 + BN + GELU, fc2 + BN + residual; reference
gkgnet.py:46-72) as one launch that keeps the hidden matrix on chip, and its dispatch from ``fused.ffn_forward`` under
GKG_ENABLE=lin_bf16,ffn_bf16.

The contract is bit identity with the two gkg_linear_bf16 launches it replaces (same contraction order on the same MFMA, same
helpers for the hidden's activation and rounding): ``torch.equal`` on the integer views, no tolerance.  Independently of the second
kernel, the outputs are held to fc2's definition in fp64 on the first launch's bf16 hidden, with the derived bounds of
tests/test_hip_linear_bf16.py."""
import functools
import itertools

import pytest
import torch

from tests.test_hip_linear_bf16 import BF16, UNSUPPORTED, _TorchProxy, _call, _check, _definition, _planes

pytestmark = pytest.mark.gpu

# (R, cin, hid, cout): one element; partial row tiles of 1, 2, 3 tiles at every model width of the envelope (80, 96, 160, 192);
# cin != cout with a hidden that is no multiple of 16, 32 or 64; a hidden of one chunk and a bit; 17 row tiles (every XCD, a tail)
SHAPES = [(1, 16, 8, 16), (127, 80, 320, 80), (129, 96, 384, 96), (257, 160, 640, 160), (130, 192, 768, 192), (65, 96, 200, 80),
          (64, 80, 72, 80), (2049, 80, 320, 80),
          (66, 80, 136, 192), (70, 192, 72, 16)]      # narrow in, wide out / wide in, one output block: the wide form's other tile shapes
FULL = [(65, 96, 200, 80), (130, 192, 768, 192)]
MODEL = (True, True, True, 1, "both")      # a1 given, a2 given, residual, GELU, both outputs
S32, S16 = 0x7FC12345, 0x7FD5              # NaN patterns no kernel writes


@functools.lru_cache(maxsize=None)
def _problem(R, cin, hid, cout):
    g = torch.Generator().manual_seed(7 + 1000 * cin + 10 * hid + cout + R)
    x = torch.randn(R, cin, generator=g).to(BF16)
    w1 = (torch.randn(hid, cin, generator=g) / cin ** 0.5).to(BF16)
    w2 = (torch.randn(cout, hid, generator=g) / hid ** 0.5).to(BF16)
    a1, c1 = torch.rand(hid, generator=g) + 0.5, torch.randn(hid, generator=g) * 0.2
    a2, c2 = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    res = torch.randn(R, cout, generator=g)
    x, w1, w2, a1, c1, a2, c2, res = (t.cuda() for t in (x, w1, w2, a1, c1, a2, c2, res))
    return dict(x=x, w1=w1, w2=w2, a1=a1, c1=c1, a2=a2, c2=c2, res=res, p1=_planes(w1), p2=_planes(w2))


def _outs(R, cout, outs):
    o32 = torch.empty(R, cout, device="cuda") if outs in ("f32", "both") else None
    o16 = torch.empty(R, cout, device="cuda", dtype=BF16) if outs in ("bf16", "both") else None
    return o32, o16


def _ffn_call(x, ldx, p1, a1, c1, p2, a2, c2, res, ldr, o32, ldo32, o16, ldo16, R, cin, hid, cout, act):
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    rc = _lib.load().gkg_ffn_bf16(_ptr(x), ldx, _ptr(p1), _ptr(a1), _ptr(c1), _ptr(p2), _ptr(a2), _ptr(c2), _ptr(res), ldr,
                                  _ptr(o32), ldo32, _ptr(o16), ldo16, R, cin, hid, cout, act, _stream())
    torch.cuda.synchronize()
    return rc


@functools.lru_cache(maxsize=None)
def _pair(shape, has_a1, has_a2, has_res, act, outs):
    """The two existing launches -> (h16, out_f32 | None, out_bf16 | None); computed once per form, never modified."""
    R, cin, hid, cout = shape
    p = _problem(*shape)
    h16 = torch.empty(R, hid, device="cuda", dtype=BF16)
    assert _call(p["x"], cin, p["p1"], p["a1"] if has_a1 else None, p["c1"], None, 0, None, 0, h16, hid, R, cin, hid, act) == 0
    o32, o16 = _outs(R, cout, outs)
    assert _call(h16, hid, p["p2"], p["a2"] if has_a2 else None, p["c2"], p["res"] if has_res else None, cout, o32, cout, o16, cout,
                 R, hid, cout, 0) == 0
    return h16, o32, o16


def _fused(shape, has_a1, has_a2, has_res, act, outs):
    R, cin, hid, cout = shape
    p = _problem(*shape)
    o32, o16 = _outs(R, cout, outs)
    rc = _ffn_call(p["x"], cin, p["p1"], p["a1"] if has_a1 else None, p["c1"], p["p2"], p["a2"] if has_a2 else None, p["c2"],
                   p["res"] if has_res else None, cout, o32, cout, o16, cout, R, cin, hid, cout, act)
    assert rc == 0
    return o32, o16


def _same_bits(got, want, what):
    for g, w, iv in zip(got, want, (torch.int32, torch.int16)):
        assert (g is None) == (w is None), what
        if g is not None:
            differ = int((g.view(iv) != w.view(iv)).sum())
            print(f"{what}: {g.dtype} elements that differ from the two launches: {differ} of {g.numel()}")
            assert torch.equal(g.view(iv), w.view(iv)), (what, differ)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bits_of_the_two_launches_in_the_form_the_model_uses(shape):
    _same_bits(_fused(shape, *MODEL), _pair(shape, *MODEL)[1:], f"{shape} model form")


@pytest.mark.parametrize("has_a,has_res,act,outs", list(itertools.product((True, False), (True, False), (0, 1), ("f32", "bf16", "both"))))
@pytest.mark.parametrize("shape", FULL, ids=str)
def test_bits_of_the_two_launches_in_every_form(shape, has_a, has_res, act, outs):
    form = (has_a, has_a, has_res, act, outs)
    _same_bits(_fused(shape, *form), _pair(shape, *form)[1:], f"{shape} a={has_a} res={has_res} act={act} {outs}")


@pytest.mark.parametrize("shape", [(65, 96, 200, 80), (257, 160, 640, 160), (130, 192, 768, 192)], ids=str)
def test_outputs_hold_fc2s_definition_on_the_first_launchs_hidden(shape):
    """Independent of the second kernel: the hidden of the FIRST launch as given operands, fc2's contract in fp64."""
    R, cin, hid, cout = shape
    p = _problem(*shape)
    h16 = _pair(shape, *MODEL)[0]
    hd, wd = h16.double().cpu(), p["w2"].double().cpu()
    want, bound = _definition(hd @ wd.t(), hd.abs() @ wd.abs().t(), hid, p["a2"].cpu(), p["c2"].cpu(), p["res"].cpu(), 0)
    o32, o16 = _fused(shape, *MODEL)
    _check(o32, o16, want, bound, f"{shape} against fc2's definition")


@pytest.mark.parametrize("shape", [(65, 96, 200, 80), (257, 160, 640, 160), (2049, 80, 320, 80)], ids=str)
def test_pitches_and_bounds(shape):
    """Row pitches above the widths, x and res column slices of wider tensors, outputs inside sentinel-filled guards: the guards
    keep their bits and the payload equals the dense call's."""
    R, cin, hid, cout = shape
    p = _problem(*shape)
    d32, d16 = _fused(shape, *MODEL)
    xw = torch.zeros(R, cin + 24, device="cuda", dtype=BF16)
    xw[:, 8:8 + cin] = p["x"]
    xw[:, :8] = 7.0
    xw[:, 8 + cin:] = -5.0                                       # neighbours of the slice must not leak into the contraction
    rw = torch.full((R, cout + 12), 3.0, device="cuda")
    rw[:, 4:4 + cout] = p["res"]
    g32 = torch.full((R + 2, cout + 8), S32, device="cuda", dtype=torch.int32)
    g16 = torch.full((R + 2, cout + 8), S16, device="cuda", dtype=torch.int16)
    rc = _ffn_call(xw[:, 8:], cin + 24, p["p1"], p["a1"], p["c1"], p["p2"], p["a2"], p["c2"], rw[:, 4:], cout + 12, g32, cout + 8,
                   g16, cout + 8, R, cin, hid, cout, 1)
    assert rc == 0
    assert torch.equal(g32[:R, :cout], d32.view(torch.int32)) and torch.equal(g16[:R, :cout], d16.view(torch.int16))
    assert bool((g32[R:] == S32).all()) and bool((g32[:, cout:] == S32).all())
    assert bool((g16[R:] == S16).all()) and bool((g16[:, cout:] == S16).all())


def _too_wide():
    """The first width (640, doubling) the library's predicate refuses."""
    from gkgnet_amd import _lib
    C = 640
    while _lib.load().gkg_ffn_bf16_supported(65, C, 80, C, 1, 1, 1, 1):
        C *= 2
    return C


@pytest.mark.parametrize("case", ["cin=12", "hid=20", "too wide"])
def test_unsupported_problems_launch_nothing(case):
    from gkgnet_amd import _lib
    R = 65
    cin, hid, cout = {"cin=12": (12, 80, 80), "hid=20": (80, 20, 80)}.get(case) or (_too_wide(), 80, _too_wide())
    W = max(96, cin, cout)
    assert _lib.load().gkg_ffn_bf16_supported(R, cin, hid, cout, 1, 1, 1, 1) == 0
    x = torch.zeros(R, W, device="cuda", dtype=BF16)
    planes = torch.zeros(W // 8, W, 8, device="cuda", dtype=BF16)
    a = torch.ones(W, device="cuda")
    res = torch.zeros(R, W, device="cuda")
    g32 = torch.full((R, W), S32, device="cuda", dtype=torch.int32)
    g16 = torch.full((R, W), S16, device="cuda", dtype=torch.int16)
    rc = _ffn_call(x, W, planes, a, a, planes, a, a, res, W, g32, W, g16, W, R, cin, hid, cout, 1)
    assert rc == UNSUPPORTED == _lib.ERR_UNSUPPORTED
    assert bool((g32 == S32).all()) and bool((g16 == S16).all())      # the NaN-filled outputs stay all-NaN


def test_two_calls_give_identical_bits():
    shape = (257, 160, 640, 160)
    a, b = _fused(shape, *MODEL), _fused(shape, *MODEL)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))


# ------------------------------------------------------------------------------------------------ dispatch from the blocks
def _blocks():
    from gkgnet_amd import layers
    from gkgnet_amd.backbone import FFN
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    from tests.util import keyed_fill_
    layers.norm_cfg["type"] = "BN"
    torch.manual_seed(0)
    C, G, H, L = 160, 2, 16, 80
    g = Grapher(C, 9, 2, "mr", "gelu", "batch", True, False, 0.2, 2, n=H * H, drop_path=0.0, relative_pos=True,
                use_multi_group=True, num_group=G)
    ffn = FFN(C, 4 * C, act="gelu")
    wide = FFN(640, 2560, act="gelu")
    gl = GrapherLabel(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, drop_path=0.0, relative_pos=False,
                      num_nodes=L, use_multi_group=True, num_group=G)
    for m in (g, ffn, wide, gl):
        sd = m.state_dict()
        keyed_fill_(sd)
        m.load_state_dict(sd)
        m.cuda().eval()
    x = torch.randn(2, C, H, H, device="cuda")
    e = torch.randn(2, L, C, device="cuda")
    return g, ffn, wide, gl, x, e


def _instrument(monkeypatch):
    """Counting wrappers around linear_bf16_eval and ffn_bf16_eval, the two affine entry points and the library GEMMs of ``fused``."""
    from gkgnet_amd import _lib, fused
    calls, counts = {"lin": 0, "ffn": 0}, {}
    real_lin, real_ffn = fused.linear_bf16_eval, fused.ffn_bf16_eval

    def lin(*a, **k):
        calls["lin"] += 1
        return real_lin(*a, **k)

    def ffn(*a, **k):
        calls["ffn"] += 1
        return real_ffn(*a, **k)
    monkeypatch.setattr(fused, "linear_bf16_eval", lin)
    monkeypatch.setattr(fused, "ffn_bf16_eval", ffn)
    lib = _lib.load()
    for name in ("gkg_affine_act", "gkg_affine_act_dual"):
        def counted(*a, _real=getattr(lib, name), _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    monkeypatch.setattr(fused, "torch", _TorchProxy(counts))
    return calls, counts


def test_block_dispatch_runs_the_ffn_as_one_launch_with_the_pairs_bits(monkeypatch):
    """Grapher + FFN on the channels-last chain, eval, bf16 autocast, gradients off, LIN_BF16 on."""
    from gkgnet_amd import fused
    g, ffn, _, _, x, _ = _blocks()
    xcl = x.to(memory_format=torch.channels_last)
    calls, counts = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "LIN_BF16", True)
    got = {}
    for on in (False, True):
        monkeypatch.setattr(fused, "FFN_BF16", on)
        calls.update(lin=0, ffn=0)
        counts.clear()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            o = ffn(g(xcl))
        assert (calls["lin"], calls["ffn"]) == ((2, 1) if on else (4, 0)), calls
        assert all(counts.get(n, 0) == 0 for n in ("mm", "addmm", "_addmm_activation", "gkg_affine_act", "gkg_affine_act_dual")), counts
        assert o.dtype == torch.float32 and o.shape == x.shape and fused.is_channels_last(o)
        ent = getattr(o, "_gkg_bf16", None)
        assert ent is not None and ent[0] == o._version and ent[1].dtype == BF16
        got[on] = (o, ent[1])
    assert torch.equal(got[True][0].view(torch.int32), got[False][0].view(torch.int32))
    assert torch.equal(got[True][1].view(torch.int16), got[False][1].view(torch.int16))


def test_forms_outside_the_dispatch_keep_their_path_bit_for_bit(monkeypatch):
    """An FFN wider than the envelope, an NCHW-contiguous input and a GrapherLabel make no ffn_bf16_eval call with the switch on and
    return the switch-off bits."""
    from gkgnet_amd import fused
    _, ffn, wide, gl, x, e = _blocks()
    calls, _ = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "LIN_BF16", True)
    feats = x.to(memory_format=torch.channels_last)
    xw = torch.randn(2, 640, 6, 6, device="cuda").to(memory_format=torch.channels_last)
    got = {}
    for on in (False, True):
        monkeypatch.setattr(fused, "FFN_BF16", on)
        calls.update(lin=0, ffn=0)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            o_wide = wide(xw)
            assert calls["lin"] == 2                                # the pair, on the own kernel
            o_nchw = ffn(x)
            e2, idx = gl(e, feats)
        assert calls["ffn"] == 0, calls
        got[on] = (o_wide, o_nchw, e2, idx)
    for t_off, t_on in zip(got[False], got[True]):
        assert t_off.dtype == t_on.dtype and torch.equal(t_off, t_on)
