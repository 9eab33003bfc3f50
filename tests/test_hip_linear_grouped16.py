"""The grouped form of the own projection kernel at the C ABI (gkg_linear_bf16_f32a_grouped / gkg_linear_f16_f32a_grouped,
csrc/gkg_linear_bf16.hip) and its thin callers (linear_bf16.train16_grouped_fwd / train16_grouped_dgrad), both element kinds:

  bits          one grouped launch against nb launches of the pinned single-matrix entry point (gkg_linear_{bf16,f16}_f32a, a = cshift
                = res = NULL, act = 0, fp32 output) on the group views, in the two layouts of the library's own caller and one with
                slack in both pitches; both sides write into buffers pre-filled with a NaN pattern no kernel writes and the WHOLE
                buffers are compared as integers — every group's tile, the slack columns and the neighbouring groups' regions.  x
                carries rounding ties in every third element, one column beyond the kind's range and (fp16) one in its subnormals:
                rounding, overflow and kept subnormals are inherited from the pinned kernel with no tolerance.
  definition    finite operands against the fp64 product of the rounded operands per group under test_hip_linear_bf16._definition
                (a = None, c = 0, no residual, no activation): |got - want| <= cin 2^-24 mag + 8 2^-24 |want|.
  refusals      every precondition of include/gkg_hip.h returns its code and leaves a sentinel-filled output untouched.
  callers       train16_grouped_fwd / train16_grouped_dgrad on a groups = 4 conv against fp64 of the rounded operands in XM column
                order (the permutation lives in the cached fragment arrays), the input gradient with contraction length co.
Reference layer: BasicConv's Conv2d(1x1, groups = 4) (torch_nn.py:57-69 behind torch_vertex.py:57-61)."""
import functools

import pytest
import torch

from tests.test_hip_linear_bf16 import _definition

pytestmark = pytest.mark.gpu

# (R, cin, cout, nb): the smallest problem; the module tests' layer (one full and one 1-row tile); stage 1 (a partial 32-column
# block); unequal widths, three groups, three row tiles; ci_pad 208 with four column tiles, the last partial; the widest stage
SHAPES = [(1, 8, 8, 1), (129, 24, 24, 4), (130, 40, 40, 4), (257, 80, 72, 3), (200, 200, 200, 4), (64, 320, 320, 4)]
LAYOUTS = ("forward", "input gradient", "slack")
KINDS = ("bf16", "f16")
S32 = 0x7FC12345                         # a NaN pattern no kernel writes
TAIL = 64                                # guard floats behind every buffer


def _lib_():
    from gkgnet_amd import _lib
    return _lib


def _kind(name):
    from gkgnet_amd import linear_bf16
    return linear_bf16.KINDS[name]


def _layout(layout, R, cin, cout, nb):
    """(ldx, x_gs, ldo, out_gs) of include/gkg_hip.h's table; "slack": the forward's x and the input gradient's out, pitches widened."""
    if layout == "forward":
        return nb * cin, cin, cout, R * cout
    if layout == "input gradient":
        return cin, R * cin, nb * cout, cout
    return nb * cin + 4, cin, nb * cout + 8, cout


def _extent(R, width, ld, gs, nb):
    return (nb - 1) * gs + (R - 1) * ld + width


def _views(flat, R, width, ld, gs, nb):
    """Group q's (R, width) matrix inside the flat buffer."""
    return [flat[q * gs:].as_strided((R, width), (ld, 1)) for q in range(nb)]


@functools.lru_cache(maxsize=None)
def _weights(kind, cin, cout, nb):
    from gkgnet_amd import derived
    k = _kind(kind)
    g = torch.Generator().manual_seed(5000 * cin + 7 * cout + nb)
    w = (torch.randn(nb, cout, cin, generator=g) / cin ** 0.5).to(k.fragment)
    planes = derived._fragments(w.cuda(), derived._up(cin, derived.K_ALIGN), derived._up(cout, derived.N_ALIGN), k.fragment)
    assert planes.numel() * 2 == nb * getattr(_lib_().load(), k.planes_bytes)(cin, cout)
    return w, planes


def _x(kind, R, cin, nb, special):
    """(nb, R, cin) fp32 on the CPU: every third element a rounding tie of the kind (the dropped mantissa bits = exactly half an ulp,
    the kept last bit as it fell); ``special``: one column beyond the kind's range and, fp16, one in its subnormals."""
    g = torch.Generator().manual_seed(9000 * cin + R + nb)
    x = torch.randn(nb, R, cin, generator=g)
    drop = 16 if kind == "bf16" else 13
    bits = x.view(torch.int32).clone()
    tie = (torch.arange(x.numel()).view(x.shape) % 3) == 0
    bits[tie] = (bits[tie] & ~((1 << drop) - 1)) | (1 << (drop - 1))
    if x.numel() >= 48:
        up = (bits[tie] >> drop) & 1
        assert bool((up == 0).any()) and bool((up == 1).any())
    x = bits.view(torch.float32).clone()
    if special:
        big, small = cin // 2, cin - 1
        huge = 3.4e38 if kind == "bf16" else 1.0e5                              # beyond bf16's 3.39e38 / fp16's 65504: +-inf
        x[..., big] = torch.where(x[..., big] < 0, -huge, huge)
        if kind == "f16":
            x[..., small] = x[..., small].sign() * x[..., small].abs().clamp(0.1, 30.0) * 2.0 ** -20
        x16 = x.to(_kind(kind).fragment)
        assert bool(torch.isinf(x16[..., big]).all())
        if kind == "f16":
            assert bool(((x16[..., small] != 0) & (x16[..., small].abs() < 2.0 ** -14)).all())
    return x


def _place(xg, R, cin, nb, ldx, x_gs):
    """The groups' matrices in one flat device buffer with the layout's pitches; everything between them is NaN."""
    flat = torch.full((_extent(R, cin, ldx, x_gs, nb) + TAIL,), float("nan"))
    for q, v in enumerate(_views(flat, R, cin, ldx, x_gs, nb)):
        v.copy_(xg[q])
    return flat.cuda()


def _out(R, cout, nb, ldo, out_gs):
    return torch.full((_extent(R, cout, ldo, out_gs, nb) + TAIL,), S32, dtype=torch.int32, device="cuda")


def _grouped(kind, x, ldx, x_gs, planes, out, ldo, out_gs, R, cin, cout, nb):
    from gkgnet_amd.ops import _ptr, _stream
    rc = getattr(_lib_().load(), _kind(kind).f32a_grouped)(_ptr(x), ldx, x_gs, _ptr(planes), _ptr(out), ldo, out_gs, R, cin, cout, nb,
                                                          _stream())
    torch.cuda.synchronize()
    return rc


def _single(kind, x, ldx, planes, out, ldo, R, cin, cout):
    from gkgnet_amd.ops import _ptr, _stream
    rc = getattr(_lib_().load(), _kind(kind).f32a)(_ptr(x), ldx, _ptr(planes), None, None, None, 0, _ptr(out), ldo, None, 0, R, cin, cout,
                                                  0, _stream())
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------ bits of the single-matrix kernel
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_launch_has_the_bits_of_the_single_matrix_kernel(kind, shape, layout):
    R, cin, cout, nb = shape
    ldx, x_gs, ldo, out_gs = _layout(layout, R, cin, cout, nb)
    _, planes = _weights(kind, cin, cout, nb)
    x = _place(_x(kind, R, cin, nb, special=True), R, cin, nb, ldx, x_gs)
    got, want = _out(R, cout, nb, ldo, out_gs), _out(R, cout, nb, ldo, out_gs)
    assert _grouped(kind, x, ldx, x_gs, planes, got, ldo, out_gs, R, cin, cout, nb) == 0
    for q in range(nb):
        assert _single(kind, x[q * x_gs:], ldx, planes[q], want[q * out_gs:], ldo, R, cin, cout) == 0
    assert torch.equal(got, want)                                                # the whole buffers, as integers
    written = torch.zeros_like(got, dtype=torch.bool)
    for v in _views(written, R, cout, ldo, out_gs, nb):
        v.fill_(True)
    assert bool((got[written] != S32).all()) and bool((got[~written] == S32).all())      # every element of every group, nothing else
    assert int(written.sum()) == nb * R * cout                                           # (the groups' regions are disjoint)
    if cin >= 16:
        assert not bool(torch.isfinite(got[written].view(torch.float32)).all())          # the overflow column reached the outputs


# ------------------------------------------------------------------------------------------------ definition
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_launch_matches_its_definition(kind, shape):
    R, cin, cout, nb = shape
    ldx, x_gs, ldo, out_gs = _layout("forward", R, cin, cout, nb)
    w, planes = _weights(kind, cin, cout, nb)
    xg = _x(kind, R, cin, nb, special=False)
    out = _out(R, cout, nb, ldo, out_gs)
    assert _grouped(kind, _place(xg, R, cin, nb, ldx, x_gs), ldx, x_gs, planes, out, ldo, out_gs, R, cin, cout, nb) == 0
    got = out[:nb * R * cout].view(torch.float32).view(nb, R, cout).double().cpu()
    xd, wd = xg.to(_kind(kind).fragment).double(), w.double()
    worst = 0.0
    for q in range(nb):
        want, bound = _definition(xd[q] @ wd[q].t(), xd[q].abs() @ wd[q].abs().t(), cin, None, torch.zeros(cout), None, 0)
        err = (got[q] - want).abs()
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
        assert bool((err <= bound).all()), (kind, shape, q, worst)
    print(f"{kind} grouped {shape}: worst err / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ refusals
def _codes():
    k = _lib_()._K
    return k["ERR_NULL"], k["ERR_SHAPE"], k["ERR_UNSUPPORTED"]


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_return_their_codes_and_write_nothing(kind):
    NULL, SHAPE, UNSUP = _codes()
    R, cin, cout, nb = 129, 24, 24, 4
    _, planes = _weights(kind, cin, cout, nb)
    x = torch.randn(R * nb * cin + 4 * TAIL, device="cuda")
    out = torch.full((R * nb * cout + 4 * TAIL,), S32, dtype=torch.int32, device="cuda")
    ldx, x_gs, ldo, out_gs = nb * cin, cin, nb * cout, cout
    base = dict(x=x, ldx=ldx, x_gs=x_gs, planes=planes, out=out, ldo=ldo, out_gs=out_gs, R=R, cin=cin, cout=cout, nb=nb)
    cases = [
        ("cin % 8", dict(cin=20), UNSUP), ("cout % 8", dict(cout=20), UNSUP),
        ("ldx % 4", dict(ldx=ldx + 2), UNSUP), ("ldo % 4", dict(ldo=ldo + 2), UNSUP),
        ("x_gs % 4", dict(x_gs=cin + 2), UNSUP), ("out_gs % 4", dict(out_gs=cout + 2), UNSUP),
        ("x alignment", dict(x=x[1:]), UNSUP), ("out alignment", dict(out=out[1:]), UNSUP),
        ("planes alignment", dict(planes=planes.view(-1)[4:]), UNSUP),
        ("nb = 0", dict(nb=0), UNSUP), ("nb = 65", dict(nb=65), UNSUP),
        ("nb x tiles", dict(R=0x7FFFFFFF, cin=8, cout=8, nb=64, ldx=512, x_gs=8, ldo=512, out_gs=8), UNSUP),
        ("ldx < cin", dict(ldx=cin - 8, nb=1), SHAPE), ("ldo < cout", dict(ldo=cout - 8, nb=1), SHAPE),
        ("R = 0", dict(R=0), SHAPE), ("cin = 0", dict(cin=0), SHAPE), ("cout = 0", dict(cout=0), SHAPE), ("R < 0", dict(R=-3), SHAPE),
        ("x_gs < 0", dict(x_gs=-cin), SHAPE),
        ("null x", dict(x=None), NULL), ("null planes", dict(planes=None), NULL), ("null out", dict(out=None), NULL),
    ]
    for what, change, code in cases:
        a = dict(base, **change)
        rc = _grouped(kind, a["x"], a["ldx"], a["x_gs"], a["planes"], a["out"], a["ldo"], a["out_gs"], a["R"], a["cin"], a["cout"], a["nb"])
        assert rc == code, (what, rc, code)
        assert bool((out == S32).all()), what
    assert _grouped(kind, x, ldx, x_gs, planes, out, ldo, out_gs, R, cin, cout, nb) == 0         # the base call itself is fine
    assert bool((out[:R * nb * cout] != S32).all()) and bool((out[R * nb * cout:] == S32).all())


# ------------------------------------------------------------------------------------------------ thin callers
def _conv(ci, co, seed):
    conv = torch.nn.Conv2d(4 * ci, 4 * co, 1, groups=4)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(4 * co, ci, 1, 1, generator=g) / ci ** 0.5)
    return conv.cuda()


CALLER_SHAPES = [(129, 24, 24), (130, 40, 24), (200, 200, 200), (64, 320, 320)]          # (R, ci, co)


@pytest.mark.parametrize("shape", CALLER_SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_dgrad_matches_fp64_of_the_rounded_operands_in_xm_order(kind, shape):
    from gkgnet_amd import fused, linear_bf16
    k = _kind(kind)
    R, ci, co = shape
    conv = _conv(ci, co, 31 * ci + co)
    dY = torch.randn(4, R, co, generator=torch.Generator().manual_seed(R + co)).cuda()
    dXM = linear_bf16.train16_grouped_dgrad(k, dY, conv)
    torch.cuda.synchronize()
    assert dXM.dtype == torch.float32 and tuple(dXM.shape) == (R, 4 * ci)
    Wp = fused._kperm_weight(conv.weight.detach().view(4, co, ci)).to(k.fragment).double().cpu()
    d = dY.to(k.fragment).double().cpu()
    worst = 0.0
    for q in range(4):
        want, bound = _definition(d[q] @ Wp[q], d[q].abs() @ Wp[q].abs(), co, None, torch.zeros(ci), None, 0)
        err = (dXM[:, q * ci:(q + 1) * ci].double().cpu() - want).abs()
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
        assert bool((err <= bound).all()), (kind, shape, q, worst)
    print(f"{kind} grouped dgrad {shape}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("shape", CALLER_SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_fwd_matches_fp64_of_the_rounded_operands_in_xm_order(kind, shape):
    from gkgnet_amd import derived, fused, linear_bf16
    k = _kind(kind)
    R, ci, co = shape
    conv = _conv(ci, co, 17 * ci + co)
    XM = torch.randn(R, 4 * ci, generator=torch.Generator().manual_seed(R + ci)).cuda()
    Y = linear_bf16.train16_grouped_fwd(k, XM, conv)
    torch.cuda.synchronize()
    assert Y.dtype == torch.float32 and tuple(Y.shape) == (4, R, co)
    assert derived.peek(conv, k.gslots[0]) is not None and derived.peek(conv, k.gslots[1]) is None
    Wp = fused._kperm_weight(conv.weight.detach().view(4, co, ci)).to(k.fragment).double().cpu()
    x = XM.to(k.fragment).double().cpu().view(R, 4, ci)
    worst = 0.0
    for q in range(4):
        want, bound = _definition(x[:, q] @ Wp[q].t(), x[:, q].abs() @ Wp[q].abs().t(), ci, None, torch.zeros(co), None, 0)
        err = (Y[q].double().cpu() - want).abs()
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
        assert bool((err <= bound).all()), (kind, shape, q, worst)
    print(f"{kind} grouped fwd {shape}: worst err / bound {worst:.3f}")
