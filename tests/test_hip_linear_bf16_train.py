"""The kernels of GKG_ENABLE=train_bf16 at the C ABI and through their thin callers (linear_bf16.py):

  gkg_linear_bf16_f32a    the projection kernel with an fp32 A operand: BIT-identical to gkg_linear_bf16 on x.to(bfloat16), in every
                          form (csrc/gkg_linear_bf16.hip: the same LDS image, contraction order and epilogue)
  train16_dgrad (bf16)    dx = bf16(dY) bf16(W) (+ residual) against the fp64 product of the rounded operands, the bound of
                          test_hip_linear_bf16._definition with the contraction length cout
  gkg_linear_wgrad_bf16   dw += bf16(dy)^T bf16(x) against fp64: |got - want| <= R 2^-24 mag + 8 2^-24 |want|, mag = |bf16(dy)|^T
                          |bf16(x)| — the first-order bound of ANY fp32 summation order over R exact products (the slabs are added
                          atomically: the order is run-dependent), the convention of _definition.
Reference layers: Conv2d(1x1) of Grapher.fc1 / fc2 (torch_vertex.py:290-306) and FFN.fc1 / fc2 (gkgnet.py:46-72)."""
import functools
import itertools

import pytest
import torch

from tests.test_hip_linear_bf16 import _definition, _planes

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SHAPES = [(1, 16, 8), (63, 80, 80), (129, 320, 80), (257, 160, 160), (300, 400, 1600), (16400, 80, 400)]
FULL = [(63, 80, 80), (257, 160, 160)]
S32, S16 = 0x7FC12345, 0x7FD5            # NaN patterns no kernel writes
# csrc/gkg_linear_bf16_train.hip: rows per LDS chunk, rows of the shortest slab, edge of a workgroup's dw tile, workgroups aimed at
WG_KC, WG_MIN_SLAB, WG_T, WG_TARGET = 32, 256, 128, 512


def _lib_():
    from gkgnet_amd import _lib
    return _lib


def _call(fn, x, ldx, planes, a, c, res, ldr, o32, ldo32, o16, ldo16, R, cin, cout, act):
    from gkgnet_amd.ops import _ptr, _stream
    rc = getattr(_lib_().load(), fn)(_ptr(x), ldx, _ptr(planes), _ptr(a), _ptr(c), _ptr(res), ldr, _ptr(o32), ldo32, _ptr(o16), ldo16,
                                    R, cin, cout, act, _stream())
    torch.cuda.synchronize()
    return rc


@functools.lru_cache(maxsize=None)
def _problem(R, cin, cout):
    """fp32 operands on the device, fixed per shape.  Every third element of x is a rounding TIE: low half 0x8000, the upper
    half's last bit as it fell (even and odd both occur: checked), so round-to-nearest-EVEN is told from round-half-up / -down."""
    g = torch.Generator().manual_seed(7000 * cin + cout + R)
    x = torch.randn(R, cin, generator=g)
    bits = x.view(torch.int32).clone()
    tie = (torch.arange(R * cin).view(R, cin) % 3) == 0
    bits[tie] = (bits[tie] & ~0xFFFF) | 0x8000
    x = bits.view(torch.float32)
    if R * cin >= 48:
        up = (bits[tie] >> 16) & 1
        assert bool((up == 0).any()) and bool((up == 1).any())
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(BF16)
    a = torch.rand(cout, generator=g) + 0.5
    c = torch.randn(cout, generator=g) * 0.2
    res = torch.randn(R, cout, generator=g)
    x, w, a, c, res = (t.cuda() for t in (x, w, a, c, res))
    return x, x.to(BF16), _planes(w), a, c, res


def _pair(shape, has_a, has_res, act, outs, zero_c=False):
    """The fp32-A call and the bf16 call on the rounded x: both outputs' bits must be equal."""
    R, cin, cout = shape
    x, x16, planes, a, c, res = _problem(*shape)
    got = []
    for fn, xin in (("gkg_linear_bf16_f32a", x), ("gkg_linear_bf16", x16)):
        o32 = torch.full((R, cout), S32, device="cuda", dtype=torch.int32) if outs in ("f32", "both") else None
        o16 = torch.full((R, cout), S16, device="cuda", dtype=torch.int16) if outs in ("bf16", "both") else None
        cs = torch.zeros_like(c) if zero_c else c
        if zero_c and fn == "gkg_linear_bf16_f32a":
            cs = None                                                            # NULL = zero, the new entry point only
        assert _call(fn, xin, cin, planes, a if has_a else None, cs, res if has_res else None, cout, o32, cout, o16, cout,
                     R, cin, cout, act) == 0
        got.append((o32, o16))
    for u, v in zip(*got):
        if u is not None:
            assert torch.equal(u, v), (shape, has_a, has_res, act, outs)
            assert not bool((u == (S32 if u.dtype == torch.int32 else S16)).any())          # everything was written
    return got[0]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_f32a_equals_the_bf16_kernel_on_the_rounded_operand(shape):
    _pair(shape, True, True, 1, "both")
    _pair(shape, False, False, 0, "f32")                                         # the form training uses


@pytest.mark.parametrize("has_a,has_res,act,outs", list(itertools.product((True, False), (True, False), (0, 1), ("f32", "bf16", "both"))))
@pytest.mark.parametrize("shape", FULL, ids=str)
def test_f32a_equals_the_bf16_kernel_in_every_form(shape, has_a, has_res, act, outs):
    _pair(shape, has_a, has_res, act, outs)


@pytest.mark.parametrize("shape", [(63, 80, 80), (300, 400, 1600)], ids=str)
def test_f32a_null_shift_is_a_zero_vector(shape):
    _pair(shape, False, False, 0, "f32", zero_c=True)
    _pair(shape, True, True, 1, "both", zero_c=True)


@pytest.mark.parametrize("shape", [(257, 160, 160), (16400, 80, 400)], ids=str)
def test_f32a_pitches_and_bounds(shape):
    """x and res as column slices of wider tensors with loud neighbours, outputs inside sentinel guards: the payload equals the
    packed call's and the guards keep their bits."""
    R, cin, cout = shape
    x, _, planes, a, c, res = _problem(*shape)
    p32, p16 = _pair(shape, True, True, 1, "both")
    xw = torch.full((R, cin + 20), 7.0e30, device="cuda")
    xw[:, 4:4 + cin] = x
    xw[:, 4 + cin:] = float("nan")
    rw = torch.full((R, cout + 12), 3.0, device="cuda")
    rw[:, 4:4 + cout] = res
    g32 = torch.full((R + 2, cout + 8), S32, device="cuda", dtype=torch.int32)
    g16 = torch.full((R + 2, cout + 8), S16, device="cuda", dtype=torch.int16)
    assert _call("gkg_linear_bf16_f32a", xw[:, 4:], cin + 20, planes, a, c, rw[:, 4:], cout + 12, g32, cout + 8, g16, cout + 8,
                 R, cin, cout, 1) == 0
    assert torch.equal(g32[:R, :cout], p32) and torch.equal(g16[:R, :cout], p16)
    assert bool((g32[R:] == S32).all()) and bool((g32[:, cout:] == S32).all())
    assert bool((g16[R:] == S16).all()) and bool((g16[:, cout:] == S16).all())
    # ldx % 4 != 0 is refused with nothing launched
    g32.fill_(S32)
    assert _call("gkg_linear_bf16_f32a", xw[:, 4:], cin + 21, planes, a, c, None, 0, g32, cout + 8, None, 0, R - 1, cin, cout,
                 0) == _lib_().ERR_UNSUPPORTED
    assert bool((g32 == S32).all())


# ------------------------------------------------------------------------------------------------ input gradient
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
    dx = linear_bf16.train16_dgrad(linear_bf16.BF16, dY, conv, residual=res)
    torch.cuda.synchronize()
    assert dx.dtype == torch.float32 and tuple(dx.shape) == (R, cin)
    d = dY.to(BF16).double().cpu()
    w = conv.weight.detach().reshape(cout, cin).to(BF16).double().cpu()
    zero = torch.zeros(cin)
    want, bound = _definition(d @ w, d.abs() @ w.abs(), cout, None, zero, None if res is None else res.cpu(), 0)
    err = (dx.double().cpu() - want).abs()
    print(f"dgrad {shape} res={with_res}: max err {err.max().item():.3e}, max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad(dy, ldg, x, ldx, dw, R, cin, cout):
    from gkgnet_amd.ops import _ptr, _stream
    rc = _lib_().load().gkg_linear_wgrad_bf16(_ptr(dy), ldg, _ptr(x), ldx, _ptr(dw), R, cin, cout, _stream())
    torch.cuda.synchronize()
    return rc


def _slabs(R, cin, cout):
    """The kernel's launch plan (wg_plan), restated to name the row counts below."""
    tiles = -(-cout // WG_T) * -(-cin // WG_T)
    slabs = min(-(-WG_TARGET // tiles), -(-R // WG_MIN_SLAB))
    rows = -(-(-(-R // slabs)) // WG_KC) * WG_KC
    return -(-R // rows), rows


@functools.lru_cache(maxsize=None)
def _wproblem(R, cin, cout):
    g = torch.Generator().manual_seed(17 * R + 3 * cin + cout)
    dy = torch.randn(R, cout, generator=g)
    x = torch.randn(R, cin, generator=g)
    d, xx = dy.to(BF16).double(), x.to(BF16).double()
    want = d.t() @ xx
    mag = d.abs().t() @ xx.abs()
    bound = R * 2.0 ** -24 * mag + 8 * 2.0 ** -24 * want.abs()
    return dy.cuda(), x.cuda(), want, bound


ROWS = [1, 63, WG_KC + 1, WG_MIN_SLAB + 1, 3 * WG_MIN_SLAB + 5]
WIDTHS = [(8, 8), (80, 80), (WG_T + 8, 80), (80, WG_T + 8), (320, 80), (80, 1280)]          # (cin, cout)


def test_row_counts_cover_the_plan():
    assert _slabs(WG_KC + 1, 80, 80) == (1, 2 * WG_KC)                           # two chunks, the second with one row
    assert _slabs(WG_MIN_SLAB + 1, 80, 80)[0] == 2                               # one slab plus one row
    assert all(_slabs(3 * WG_MIN_SLAB + 5, ci, co)[0] >= 3 for ci, co in WIDTHS)
    assert max(ROWS) <= 16400


@pytest.mark.parametrize("widths", WIDTHS, ids=str)
@pytest.mark.parametrize("R", ROWS)
def test_wgrad_matches_fp64_within_the_summation_bound(R, widths):
    cin, cout = widths
    dy, x, want, bound = _wproblem(R, cin, cout)
    dw = torch.zeros(cout, cin, device="cuda")
    assert _wgrad(dy, cout, x, cin, dw, R, cin, cout) == 0
    err = (dw.double().cpu() - want).abs()
    print(f"wgrad R={R} cin={cin} cout={cout} slabs={_slabs(R, cin, cout)}: max err {err.max().item():.3e}, "
          f"max err / bound {(err / bound.clamp_min(1e-300)).max().item():.4f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("R", [63, 3 * WG_MIN_SLAB + 5])
def test_wgrad_adds_to_what_dw_holds(R):
    """dw prefilled with random values comes back as prefill + product within the bound plus one rounding (of the result: half an
    ulp, 2^-24 relative).  With one slab (R = 63) that is exact arithmetic: one atomic add per element, got = fl(prefill + partial);
    with four slabs each element takes four adds, which the R 2^-24 mag term of the bound covers many times over."""
    cin, cout = WG_T + 8, 80
    dy, x, want, bound = _wproblem(R, cin, cout)
    pre = torch.randn(cout, cin, generator=torch.Generator().manual_seed(R))
    dw = pre.cuda()
    assert _wgrad(dy, cout, x, cin, dw, R, cin, cout) == 0
    total = pre.double() + want
    err = (dw.double().cpu() - total).abs()
    tol = bound + 2.0 ** -24 * (total.abs() + bound)
    print(f"wgrad accumulate R={R}: max err / tol {(err / tol.clamp_min(1e-300)).max().item():.4f}")
    assert bool((err <= tol).all())


def test_wgrad_guards():
    """Operands as column slices of wider tensors with loud neighbours, over-allocated rows >= R full of NaN, dw inside a
    sentinel-filled frame: the product equals the packed call's within the bound, the frame keeps its bits."""
    R, cin, cout = 3 * WG_MIN_SLAB + 5, 80, WG_T + 8
    dy, x, want, bound = _wproblem(R, cin, cout)
    dyw = torch.full((R + 40, cout + 12), 1.0e30, device="cuda")
    dyw[:R, 4:4 + cout] = dy
    dyw[R:] = float("nan")
    xw = torch.full((R + 40, cin + 8), -1.0e30, device="cuda")
    xw[:R, 4:4 + cin] = x
    xw[R:] = float("nan")
    frame = torch.full((cout * cin + 128,), S32, device="cuda", dtype=torch.int32)
    dw = frame[64:64 + cout * cin].view(torch.float32).view(cout, cin)
    dw.zero_()
    assert _wgrad(dyw[:, 4:], cout + 12, xw[:, 4:], cin + 8, dw, R, cin, cout) == 0
    err = (dw.double().cpu() - want).abs()
    assert bool(torch.isfinite(dw).all()) and bool((err <= bound).all())
    assert bool((frame[:64] == S32).all()) and bool((frame[64 + cout * cin:] == S32).all())


@pytest.mark.parametrize("cin,cout,ldg,ldx", [(12, 80, 96, 96), (80, 20, 96, 96), (80, 80, 72, 96), (80, 80, 96, 72),
                                              (80, 80, 98, 96), (80, 80, 96, 90)])
def test_wgrad_unsupported_problems_launch_nothing(cin, cout, ldg, ldx):
    R = 65
    dy = torch.ones(R, 100, device="cuda")
    x = torch.ones(R, 100, device="cuda")
    dw = torch.full((96 * 96,), S32, device="cuda", dtype=torch.int32)
    assert _wgrad(dy, ldg, x, ldx, dw, R, cin, cout) == _lib_().ERR_UNSUPPORTED
    assert bool((dw == S32).all())
    if cin % 8 or cout % 8:
        assert _lib_().load().gkg_linear_wgrad_bf16_supported(R, cin, cout) == 0


def test_wgrad_caller_zeroes_or_trusts_the_slot():
    """linear_bf16_wgrad's ``out``: a fresh tensor without one, a dirty slot is cleared, a slot marked ``_gkg_zero`` is trusted."""
    from gkgnet_amd import linear_bf16
    R, cin, cout = 63, 80, 80
    dy, x, want, bound = _wproblem(R, cin, cout)
    fresh = linear_bf16.linear_bf16_wgrad(dy, x)
    dirty = torch.full((cout, cin), 5.0, device="cuda")
    assert linear_bf16.linear_bf16_wgrad(dy, x, dirty) is dirty
    clean = torch.zeros(cout, cin, device="cuda")
    clean._gkg_zero = True
    assert linear_bf16.linear_bf16_wgrad(dy, x, clean) is clean
    torch.cuda.synchronize()
    for t in (fresh, dirty, clean):
        assert bool(((t.double().cpu() - want).abs() <= bound).all())
