"""The kernel of GKG_ENABLE=train_f16 at the C ABI and through its thin callers (linear_bf16.py):

  gkg_linear_f16_f32a   the projection kernel's fp16 instantiation with an fp32 A operand (csrc/gkg_linear_bf16.hip): the fp32
                        accumulation of the exact products of f16(x) and the fp16 fragments.
    rounding            the call on x and the call on x.to(float16).float() give equal bits, on an x whose every third element is an
                        fp16 rounding TIE (low 13 mantissa bits 0x1000, bit 13 of both parities), with one column scaled beyond
                        fp16's range (-> inf) and one into its subnormals: round-to-nearest-even is told from half-up / truncation,
                        overflow to inf from clamping, kept subnormals from flushing — without a second kernel.
    definition          finite problems against the fp64 product of the fp16-rounded operands under the bound of
                        test_hip_linear_bf16._definition (an fp16 x fp16 product is exact in fp32: 22 significand bits, exponents
                        within fp32's range — the derivation holds as it stands):
                          |got - want| <= cin 2^-24 |a| mag + 8 2^-24 (|want| + |res|) + 3e-7 |z| [GELU].
                        An all-subnormal x must meet the same bound (a flushing operand path would return zeros).
  train16_dgrad (f16)   dx = f16(dY) f16(W) (+ residual) against fp64 of the rounded operands, contraction length cout.
Reference layers: Conv2d(1x1) of Grapher.fc1 / fc2 (torch_vertex.py:290-306) and FFN.fc1 / fc2 (gkgnet.py:46-72) under fp16 AMP
(configs/gkgnet/gkgnet_coco_576.py:146)."""
import functools

import pytest
import torch

from tests.test_hip_linear_bf16 import _definition

pytestmark = pytest.mark.gpu

F16 = torch.float16
SHAPES = [(1, 16, 8), (63, 80, 80), (65, 40, 72), (129, 320, 80), (257, 160, 160), (300, 400, 1600)]
S32, S16 = 0x7FC12345, 0x7FD5            # NaN patterns no kernel writes


def _lib_():
    from gkgnet_amd import _lib
    return _lib


def _planes(w16):
    """fp16 weight (cout, cin) -> the fragment array [ci_pad/8][co_pad][8] (include/gkg_hip.h: paddings 16 / 32)."""
    co, ci = w16.shape
    ci_pad, co_pad = (ci + 15) // 16 * 16, (co + 31) // 32 * 32
    W = torch.zeros((co_pad, ci_pad), dtype=F16, device=w16.device)
    W[:co, :ci] = w16
    p = W.view(co_pad, ci_pad // 8, 8).permute(1, 0, 2).contiguous()
    assert p.numel() * 2 == _lib_().load().gkg_linear_f16_planes_bytes(ci, co)
    return p


def _call(x, ldx, planes, a, c, res, ldr, o32, ldo32, o16, ldo16, R, cin, cout, act):
    from gkgnet_amd.ops import _ptr, _stream
    rc = _lib_().load().gkg_linear_f16_f32a(_ptr(x), ldx, _ptr(planes), _ptr(a), _ptr(c), _ptr(res), ldr, _ptr(o32), ldo32, _ptr(o16),
                                            ldo16, R, cin, cout, act, _stream())
    torch.cuda.synchronize()
    return rc


def _ties(x):
    """Every third element an fp16 rounding tie: the 13 mantissa bits fp16 drops set to 0x1000, bit 13 as it fell."""
    bits = x.view(torch.int32).clone()
    tie = (torch.arange(x.numel()).view(x.shape) % 3) == 0
    bits[tie] = (bits[tie] & ~0x1FFF) | 0x1000
    return bits.view(torch.float32), bits, tie


@functools.lru_cache(maxsize=None)
def _problem(R, cin, cout):
    """Finite operands (CPU + device, fixed per shape), with ties in x, and the fp64 contraction of the ROUNDED operands with its
    absolute-value twin, computed once per shape."""
    g = torch.Generator().manual_seed(9000 * cin + cout + R)
    x, bits, tie = _ties(torch.randn(R, cin, generator=g))
    if R * cin >= 48:
        up = (bits[tie] >> 13) & 1
        assert bool((up == 0).any()) and bool((up == 1).any())
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(F16)
    a = torch.rand(cout, generator=g) + 0.5
    c = torch.randn(cout, generator=g) * 0.2
    res = torch.randn(R, cout, generator=g)
    xd, wd = x.to(F16).double(), w.double()
    acc, mag = xd @ wd.t(), xd.abs() @ wd.abs().t()
    dev = tuple(t.cuda() for t in (x, w, a, c, res))
    return (x, w, a, c, res), (acc, mag), dev + (_planes(dev[1]),)


def _outs(R, cout, outs):
    o32 = torch.full((R, cout), S32, device="cuda", dtype=torch.int32) if outs in ("f32", "both") else None
    o16 = torch.full((R, cout), S16, device="cuda", dtype=torch.int16) if outs in ("f16", "both") else None
    return o32, o16


# ------------------------------------------------------------------------------------------------ rounding
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_rounding_is_torchs_fp16_cast(shape):
    R, cin, cout = shape
    _, _, (x, w, a, c, res, planes) = _problem(*shape)
    x = x.clone()
    big, small = cin // 2, cin - 1
    x[:, big] = torch.where(x[:, big] < 0, -1.0e5, 1.0e5)                        # beyond 65504: +-inf in fp16
    x[:, small] = x[:, small].sign() * x[:, small].abs().clamp(0.1, 30.0) * 2.0 ** -20     # fp16 subnormals: 2^-24 <= |x| < 2^-14
    x16 = x.to(F16)
    assert bool(torch.isinf(x16[:, big]).all()) and bool(((x16[:, small] != 0) & (x16[:, small].abs() < 2.0 ** -14)).all())
    got = []
    for xin in (x, x16.float()):
        o32, o16 = _outs(R, cout, "both")
        assert _call(xin, cin, planes, a, c, res, cout, o32, cout, o16, cout, R, cin, cout, 0) == 0
        got.append((o32, o16))
    (p32, p16), (q32, q16) = got
    assert torch.equal(p32, q32) and torch.equal(p16, q16)                        # as bits: inf / NaN patterns included
    assert not bool((p32 == S32).any()) and not bool((p16 == S16).any())
    assert not bool(torch.isfinite(p32.view(torch.float32)).all())                # the inf column reached the rows that hold it
    # the subnormal column alone (every other column of x zero): its products are there, exactly
    xs = torch.zeros_like(x)
    xs[:, small] = x[:, small]
    o32, _ = _outs(R, cout, "f32")
    assert _call(xs, cin, planes, None, None, None, 0, o32, cout, None, 0, R, cin, cout, 0) == 0
    want = x16[:, small].double().view(R, 1) * w[:, small].double().view(1, cout)          # one exact product per element
    assert torch.equal(o32.view(torch.float32).double(), want) and bool((want != 0).any())


# ------------------------------------------------------------------------------------------------ definition
FORMS = {"a+res+gelu, both": (True, True, 1, "both"), "plain, fp32": (False, False, 0, "f32")}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_matches_its_definition(shape, form):
    has_a, has_res, act, outs = FORMS[form]
    R, cin, cout = shape
    (_, _, a_c, c_c, res_c), (acc, mag), (x, w, a, c, res, planes) = _problem(*shape)
    o32, o16 = _outs(R, cout, outs)
    assert _call(x, cin, planes, a if has_a else None, c, res if has_res else None, cout, o32, cout, o16, cout, R, cin, cout, act) == 0
    want, bound = _definition(acc, mag, cin, a_c if has_a else None, c_c, res_c if has_res else None, act)
    got = o32.view(torch.float32)
    err = (got.double().cpu() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"f16 {shape} {form}: max err {err.max().item():.3e}, worst err / bound {worst:.3f}")
    assert bool((err <= bound).all()), (shape, form, worst)
    if o16 is not None:
        assert torch.equal(got.to(F16).view(torch.int16), o16)                   # the fp16 output is the rounding of the fp32 one


@pytest.mark.parametrize("shape", [(63, 80, 80), (300, 400, 1600)], ids=str)
def test_null_shift_is_a_zero_vector(shape):
    R, cin, cout = shape
    _, _, (x, w, a, c, res, planes) = _problem(*shape)
    for has_a, has_res, act, outs in FORMS.values():
        got = []
        for cs in (None, torch.zeros_like(c)):
            o32, o16 = _outs(R, cout, outs)
            assert _call(x, cin, planes, a if has_a else None, cs, res if has_res else None, cout, o32, cout, o16, cout, R, cin, cout,
                         act) == 0
            got.append((o32, o16))
        for u, v in zip(*got):
            if u is not None:
                assert torch.equal(u, v)


@pytest.mark.parametrize("shape", [(65, 40, 72), (257, 160, 160)], ids=str)
def test_subnormal_operands_are_not_flushed(shape):
    """x = randn 2^-18: every f16(x) is subnormal (or zero); the weights are scaled up so that the result is an ordinary fp32 number."""
    R, cin, cout = shape
    g = torch.Generator().manual_seed(77 + cin)
    x = torch.randn(R, cin, generator=g) * 2.0 ** -18
    x16 = x.to(F16)
    assert bool((x16.abs() < 2.0 ** -14).all()) and bool((x16 != 0).float().mean() > 0.9)
    w = (torch.randn(cout, cin, generator=g) * 64).to(F16)
    xd, wd = x16.double(), w.double()
    want, bound = _definition(xd @ wd.t(), xd.abs() @ wd.abs().t(), cin, None, torch.zeros(cout), None, 0)
    o32 = torch.empty(R, cout, device="cuda")
    assert _call(x.cuda(), cin, _planes(w.cuda()), None, None, None, 0, o32, cout, None, 0, R, cin, cout, 0) == 0
    err = (o32.double().cpu() - want).abs()
    print(f"f16 subnormal x {shape}: mean |want| {want.abs().mean().item():.3e}, mean |got| {o32.abs().mean().item():.3e}, "
          f"worst err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((want.abs() > 0).float().mean() > 0.9)
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------ pitches and guards
@pytest.mark.parametrize("shape", [(257, 160, 160), (16400, 80, 400)], ids=str)
def test_pitches_and_bounds(shape):
    """x and res as column slices of wider tensors with loud neighbours, outputs inside sentinel guards: the payload equals the
    packed call's and the guards keep their bits; ldx % 4 != 0 is refused with nothing written."""
    R, cin, cout = shape
    _, _, (x, w, a, c, res, planes) = _problem(*shape)
    p32, p16 = _outs(R, cout, "both")
    assert _call(x, cin, planes, a, c, res, cout, p32, cout, p16, cout, R, cin, cout, 1) == 0
    assert not bool((p32 == S32).any()) and not bool((p16 == S16).any())
    xw = torch.full((R, cin + 20), 7.0e30, device="cuda")
    xw[:, 4:4 + cin] = x
    xw[:, 4 + cin:] = float("nan")
    rw = torch.full((R, cout + 12), 3.0, device="cuda")
    rw[:, 4:4 + cout] = res
    g32 = torch.full((R + 2, cout + 8), S32, device="cuda", dtype=torch.int32)
    g16 = torch.full((R + 2, cout + 8), S16, device="cuda", dtype=torch.int16)
    assert _call(xw[:, 4:], cin + 20, planes, a, c, rw[:, 4:], cout + 12, g32, cout + 8, g16, cout + 8, R, cin, cout, 1) == 0
    assert torch.equal(g32[:R, :cout], p32) and torch.equal(g16[:R, :cout], p16)
    assert bool((g32[R:] == S32).all()) and bool((g32[:, cout:] == S32).all())
    assert bool((g16[R:] == S16).all()) and bool((g16[:, cout:] == S16).all())
    g32.fill_(S32)
    assert _call(xw[:, 4:], cin + 21, planes, a, c, None, 0, g32, cout + 8, None, 0, R - 1, cin, cout, 0) == _lib_().ERR_UNSUPPORTED
    assert bool((g32 == S32).all())


# ------------------------------------------------------------------------------------------------ thin callers
@pytest.mark.parametrize("with_res", (False, True))
@pytest.mark.parametrize("shape", [(65, 80, 320), (129, 320, 80), (200, 2560, 640)], ids=str)
def test_dgrad_matches_the_fp64_product_of_the_rounded_operands(shape, with_res):
    from gkgnet_amd import linear_bf16
    R, cin, cout = shape
    g = torch.Generator().manual_seed(31 * cin + cout)
    conv = torch.nn.Conv2d(cin, cout, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(cout, cin, 1, 1, generator=g) / cout ** 0.5)
    conv.cuda()
    dY = torch.randn(R, cout, generator=g).cuda()
    res = torch.randn(R, cin, generator=g).cuda() if with_res else None
    dx = linear_bf16.train16_dgrad(linear_bf16.F16, dY, conv, residual=res)
    torch.cuda.synchronize()
    assert dx.dtype == torch.float32 and tuple(dx.shape) == (R, cin)
    d = dY.to(F16).double().cpu()
    w = conv.weight.detach().reshape(cout, cin).to(F16).double().cpu()
    want, bound = _definition(d @ w, d.abs() @ w.abs(), cout, None, torch.zeros(cin), None if res is None else res.cpu(), 0)
    err = (dx.double().cpu() - want).abs()
    print(f"f16 dgrad {shape} res={with_res}: max err {err.max().item():.3e}, worst err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())


def test_train_fwd_is_the_c_call_on_the_cached_fragments():
    from gkgnet_amd import derived, linear_bf16
    R, cin, cout = 65, 40, 72
    g = torch.Generator().manual_seed(3)
    conv = torch.nn.Conv2d(cin, cout, 1).cuda()
    x = torch.randn(R, cin, generator=g).cuda()
    Y = linear_bf16.train16_fwd(linear_bf16.F16, x, conv)
    torch.cuda.synchronize()
    assert torch.equal(derived.lin_planes(conv, "f16"), _planes(conv.weight.detach().reshape(cout, cin).to(F16)))
    xd, wd = x.to(F16).double().cpu(), conv.weight.detach().reshape(cout, cin).to(F16).double().cpu()
    want, bound = _definition(xd @ wd.t(), xd.abs() @ wd.abs().t(), cin, None, torch.zeros(cout), None, 0)
    assert bool(((Y.double().cpu() - want).abs() <= bound).all())
