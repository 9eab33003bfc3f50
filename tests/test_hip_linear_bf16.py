"""gkg_linear_bf16 (csrc/gkg_linear_bf16.hip): the dense bf16 projection with eval-mode BN, GELU, the fp32 residual and both output
precisions in its epilogue, held to its definition evaluated in fp64 on the same bf16 operands, and its dispatch from
``fused._lin`` under GKG_ENABLE=lin_bf16 (reference torch_vertex.py:290-306, gkgnet.py:46-72, torch_nn.py:57-69).

Bounds (derived, not measured; every element must be within them):
  fp32 output   |got - want| <= cin 2^-24 |a| sum_k |x w|  +  8 2^-24 (|want| + |res|)  +  3e-7 |z| [act = 1]
                (any fp32 summation order of exact bf16 x bf16 products, first order; the epilogue's roundings; the shared GELU's
                documented 1.5e-7 erf error on the pre-activation z)
  bf16 output   |got - bf16(want)| <= 2^-7 |want| + 1e-3 everywhere and > 97 % equal bits (the criterion of test_hip_mrgemm.py);
                with both outputs, out_bf16 == out_f32.bfloat16() bit for bit."""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SHAPES = [(1, 16, 8), (63, 80, 80), (65, 80, 320), (129, 320, 80), (257, 160, 160), (300, 400, 1600), (200, 2560, 640),
          (324, 96, 384), (40, 3072, 768),
          (16400, 80, 400)]      # 129 row tiles x 4 column tiles: the 128-column form (full chunks, a one-step tail, an edge column tile)
FULL = [(65, 80, 320), (200, 2560, 640)]
# (a given, residual, act, outputs): Grapher.fc1, Grapher.fc2, FFN.fc1, FFN.fc2
MODEL = {"fc1": (True, False, 0, "f32"), "fc2": (True, True, 0, "both"), "ffn_fc1": (True, False, 1, "bf16"),
         "ffn_fc2": (True, True, 0, "both")}
UNSUPPORTED = -3


def _planes(w16):
    """bf16 weight (cout, cin) -> the fragment array [ci_pad/8][co_pad][8] (include/gkg_hip.h: paddings 16 / 32)."""
    from gkgnet_amd import _lib
    co, ci = w16.shape
    ci_pad, co_pad = (ci + 15) // 16 * 16, (co + 31) // 32 * 32
    W = torch.zeros((co_pad, ci_pad), dtype=BF16, device=w16.device)
    W[:co, :ci] = w16
    p = W.view(co_pad, ci_pad // 8, 8).permute(1, 0, 2).contiguous()
    assert p.numel() * 2 == _lib.load().gkg_linear_bf16_planes_bytes(ci, co)
    return p


@functools.lru_cache(maxsize=None)
def _problem(R, cin, cout):
    """Operands (CPU, fixed per shape) and the fp64 contraction with its absolute-value twin, computed once per shape."""
    g = torch.Generator().manual_seed(1000 * cin + cout + R)
    x = torch.randn(R, cin, generator=g).to(BF16)
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(BF16)
    a = torch.rand(cout, generator=g) + 0.5
    c = torch.randn(cout, generator=g) * 0.2
    res = torch.randn(R, cout, generator=g)
    acc = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()
    dev = tuple(t.cuda() for t in (x, w, a, c, res))
    return (x, w, a, c, res), (acc, mag), dev + (_planes(dev[1]),)


def _definition(acc, mag, cin, a, c, res, act):
    """The contract in fp64 -> (want, bound of the fp32 output)."""
    av = torch.ones_like(c, dtype=torch.float64) if a is None else a.double()
    z = av * acc + c.double()
    want = 0.5 * z * (1.0 + torch.special.erf(z * 0.5 ** 0.5)) if act == 1 else z.clone()
    bound = cin * 2.0 ** -24 * av.abs() * mag
    rabs = torch.zeros_like(want)
    if res is not None:
        want = want + res.double()
        rabs = res.double().abs()
    bound = bound + 8 * 2.0 ** -24 * (want.abs() + rabs)
    if act == 1:
        bound = bound + 3e-7 * z.abs()
    return want, bound


def _check(o32, o16, want, bound, what):
    if o32 is not None:
        err = (o32.double().cpu() - want).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{what}: fp32 max err {err.max().item():.3e}, max err / bound {worst:.3f}")
        assert bool((err <= bound).all()), (what, worst, int((err > bound).sum()))
    if o16 is not None:
        w16 = want.float().to(BF16)
        got = o16.cpu()
        err = (got.double() - w16.double()).abs()
        tol = 2.0 ** -7 * want.abs() + 1e-3
        same = (got.view(torch.int16) == w16.view(torch.int16)).double().mean().item()
        print(f"{what}: bf16 max err {err.max().item():.3e}, equal bits {same:.4f}")
        assert bool((err <= tol).all()), (what, err.max().item(), int((err > tol).sum()))
        assert same > 0.97, (what, same)
    if o32 is not None and o16 is not None:
        assert torch.equal(o32.to(BF16).view(torch.int16), o16.view(torch.int16)), what


def _call(x, ldx, planes, a, c, res, ldr, o32, ldo32, o16, ldo16, R, cin, cout, act):
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    rc = _lib.load().gkg_linear_bf16(_ptr(x), ldx, _ptr(planes), _ptr(a), _ptr(c), _ptr(res), ldr, _ptr(o32), ldo32, _ptr(o16),
                                     ldo16, R, cin, cout, act, _stream())
    torch.cuda.synchronize()
    return rc


def _run(shape, has_a, has_res, act, outs):
    R, cin, cout = shape
    (_, _, a_c, c_c, res_c), (acc, mag), (x, w, a, c, res, planes) = _problem(*shape)
    o32 = torch.empty(R, cout, device="cuda") if outs in ("f32", "both") else None
    o16 = torch.empty(R, cout, device="cuda", dtype=BF16) if outs in ("bf16", "both") else None
    rc = _call(x, cin, planes, a if has_a else None, c, res if has_res else None, cout, o32, cout, o16, cout, R, cin, cout, act)
    assert rc == 0
    want, bound = _definition(acc, mag, cin, a_c if has_a else None, c_c, res_c if has_res else None, act)
    _check(o32, o16, want, bound, f"{shape} a={has_a} res={has_res} act={act} {outs}")
    return o32, o16


@pytest.mark.parametrize("layer", list(MODEL))
@pytest.mark.parametrize("shape", [s for s in SHAPES if s not in FULL], ids=str)
def test_kernel_matches_its_definition_in_the_forms_the_model_uses(shape, layer):
    _run(shape, *MODEL[layer])


@pytest.mark.parametrize("has_a,has_res,act,outs", list(itertools.product((True, False), (True, False), (0, 1), ("f32", "bf16", "both"))))
@pytest.mark.parametrize("shape", FULL, ids=str)
def test_kernel_matches_its_definition_in_every_form(shape, has_a, has_res, act, outs):
    _run(shape, has_a, has_res, act, outs)


@pytest.mark.parametrize("shape", [(65, 80, 320), (257, 160, 160), (129, 320, 80), (16400, 80, 400)], ids=str)
def test_pitches_and_bounds(shape):
    """Row pitches above the widths, x and res column slices of wider tensors, outputs inside sentinel-filled guards: the guards
    keep their bits and the payload equals the packed call's."""
    R, cin, cout = shape
    _, _, (x, w, a, c, res, planes) = _problem(*shape)
    p32, p16 = _run(shape, True, True, 1, "both")
    xw = torch.zeros(R, cin + 24, device="cuda", dtype=BF16)
    xw[:, 8:8 + cin] = x
    xw[:, :8] = 7.0
    xw[:, 8 + cin:] = -5.0                                       # neighbours of the slice must not leak into the contraction
    rw = torch.full((R, cout + 12), 3.0, device="cuda")
    rw[:, 4:4 + cout] = res
    S32, S16 = 0x7FC12345, 0x7FD5      # NaN patterns no kernel writes
    g32 = torch.full((R + 2, cout + 8), S32, device="cuda", dtype=torch.int32)
    g16 = torch.full((R + 2, cout + 8), S16, device="cuda", dtype=torch.int16)
    rc = _call(xw[:, 8:], cin + 24, planes, a, c, rw[:, 4:], cout + 12, g32, cout + 8, g16, cout + 8, R, cin, cout, 1)
    assert rc == 0
    assert torch.equal(g32[:R, :cout], p32.view(torch.int32)) and torch.equal(g16[:R, :cout], p16.view(torch.int16))
    assert bool((g32[R:] == S32).all()) and bool((g32[:, cout:] == S32).all())
    assert bool((g16[R:] == S16).all()) and bool((g16[:, cout:] == S16).all())


@pytest.mark.parametrize("cin,cout", [(12, 80), (80, 20)])
def test_unsupported_problems_launch_nothing(cin, cout):
    from gkgnet_amd import _lib
    R = 65
    assert _lib.load().gkg_linear_bf16_supported(R, cin, cout, 1, 1, 1, 0) == 0
    x = torch.zeros(R, 96, device="cuda", dtype=BF16)
    planes = torch.zeros(96 // 8, 96, 8, device="cuda", dtype=BF16)
    a = torch.ones(96, device="cuda")
    res = torch.zeros(R, 96, device="cuda")
    S32, S16 = 0x7FC12345, 0x7FD5
    g32 = torch.full((R, 96), S32, device="cuda", dtype=torch.int32)
    g16 = torch.full((R, 96), S16, device="cuda", dtype=torch.int16)
    rc = _call(x, 96, planes, a, a, res, 96, g32, 96, g16, 96, R, cin, cout, 0)
    assert rc == UNSUPPORTED == _lib.ERR_UNSUPPORTED
    assert bool((g32 == S32).all()) and bool((g16 == S16).all())


def test_two_calls_give_identical_bits():
    shape = (300, 400, 1600)
    R, cin, cout = shape
    _, _, (x, w, a, c, res, planes) = _problem(*shape)
    outs = []
    for _ in range(2):
        o32 = torch.empty(R, cout, device="cuda")
        o16 = torch.empty(R, cout, device="cuda", dtype=BF16)
        assert _call(x, cin, planes, a, c, res, cout, o32, cout, o16, cout, R, cin, cout, 1) == 0
        outs.append((o32, o16))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))


# ------------------------------------------------------------------------------------------------ dispatch from the blocks
class _TorchProxy:
    """``torch`` as ``fused`` sees it, with the three library-GEMM names counted."""

    def __init__(self, counts):
        self._counts = counts

    def __getattr__(self, name):
        real = getattr(torch, name)
        if name in ("mm", "addmm", "_addmm_activation"):
            def counted(*a, **k):
                self._counts[name] = self._counts.get(name, 0) + 1
                return real(*a, **k)
            return counted
        return real


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
    gl = GrapherLabel(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, drop_path=0.0, relative_pos=False,
                      num_nodes=L, use_multi_group=True, num_group=G)
    for m in (g, ffn, gl):
        sd = m.state_dict()
        keyed_fill_(sd)
        m.load_state_dict(sd)
        m.cuda().eval()
    x = torch.randn(2, C, H, H, device="cuda")
    e = torch.randn(2, L, C, device="cuda")
    return g, ffn, gl, x, e


def _instrument(monkeypatch):
    """Counting wrappers around linear_bf16_eval (recording operands and results), the two affine entry points and the library
    GEMMs of ``fused``."""
    from gkgnet_amd import _lib, fused
    rec, counts = [], {}
    real = fused.linear_bf16_eval

    def recording(x16, conv, bn, act=0, residual=None, want_f32=True, want_bf16=False):
        o32, o16 = real(x16, conv, bn, act, residual, want_f32=want_f32, want_bf16=want_bf16)
        rec.append((x16, conv, bn, act, residual, o32, o16))
        return o32, o16
    monkeypatch.setattr(fused, "linear_bf16_eval", recording)
    lib = _lib.load()
    for name in ("gkg_affine_act", "gkg_affine_act_dual"):
        def counted(*a, _real=getattr(lib, name), _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    monkeypatch.setattr(fused, "torch", _TorchProxy(counts))
    return rec, counts


def test_block_dispatch_runs_four_own_launches_and_holds_the_definition(monkeypatch):
    """Grapher + FFN on the channels-last chain, eval, bf16 autocast, gradients off."""
    from gkgnet_amd import _lib, bn_passes, fused
    g, ffn, _, x, _ = _blocks()
    xcl = x.to(memory_format=torch.channels_last)
    with torch.no_grad():
        ref = ffn(g(xcl)).float()                                 # fp32: the path the reference fixtures pin
    rec, counts = _instrument(monkeypatch)
    outs = {}
    for on in (False, True):
        monkeypatch.setattr(fused, "LIN_BF16", on)
        rec.clear()
        counts.clear()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            o = ffn(g(xcl))
        if not on:
            assert len(rec) == 0
        else:
            assert len(rec) == 4
            assert counts.get("gkg_affine_act", 0) == 0 and counts.get("gkg_affine_act_dual", 0) == 0, counts
            assert all(counts.get(n, 0) == 0 for n in ("mm", "addmm", "_addmm_activation")), counts
            assert o.dtype == torch.float32 and o.shape == x.shape and fused.is_channels_last(o)
            ent = getattr(o, "_gkg_bf16", None)
            assert ent is not None and ent[0] == o._version and ent[1].dtype == BF16
            assert torch.equal(ent[1].view(2, 16, 16, 160).permute(0, 3, 1, 2), o.to(BF16))
        outs[on] = o.float()
    # every recorded launch against the fp64 definition, with the bounds of the kernel tests
    forms = []
    for i, (x16, conv, bn, act, res, o32, o16) in enumerate(rec):
        a, c = bn_passes.eval_ac(_lib.load(), bn, conv.bias, conv.weight.shape[0])
        xd = x16.double().cpu()
        wd = conv.weight.detach().reshape(conv.weight.shape[0], -1).to(BF16).double().cpu()
        want, bound = _definition(xd @ wd.t(), xd.abs() @ wd.abs().t(), xd.shape[1], a.cpu(), c.cpu(),
                                  None if res is None else res.cpu(), act)
        _check(o32, o16, want, bound, f"launch {i}")
        forms.append((act, res is not None, o32 is not None, o16 is not None))
    assert forms == [(0, False, True, False), (0, True, True, True), (1, False, False, True), (0, True, True, True)]
    e_on = ((outs[True] - ref).norm() / ref.norm()).item()
    e_off = ((outs[False] - ref).norm() / ref.norm()).item()
    print(f"block error against the fp32 path: lin_bf16 on {e_on:.4e}, off {e_off:.4e}")
    assert e_on <= 1.5 * e_off, (e_on, e_off)


def test_forms_outside_the_dispatch_keep_their_path_bit_for_bit(monkeypatch):
    """An NCHW-contiguous Grapher input and a GrapherLabel make no own launch with the switch on and return the switch-off bits."""
    from gkgnet_amd import fused
    g, _, gl, x, e = _blocks()
    rec, _ = _instrument(monkeypatch)
    feats = x.to(memory_format=torch.channels_last)
    got = {}
    for on in (False, True):
        monkeypatch.setattr(fused, "LIN_BF16", on)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            rec.clear()
            o = g(x)
            n_grapher = len(rec)
            e2, idx = gl(e, feats)
            n_label = len(rec) - n_grapher
        assert (n_grapher, n_label) == (0, 0)
        got[on] = (o, e2, idx)
    for t_off, t_on in zip(got[False], got[True]):
        assert t_off.dtype == t_on.dtype and torch.equal(t_off, t_on)
