"""The fp32 NCHW -> token-major re-layouts with 16-byte accesses (csrc/gkg_dense.hip nchw_to_tm_wide_kernel, taken inside
gkg_nchw_to_tm, gkg_nchw_to_tm_add and gkg_nchw_to_tm_add_bnstats) through the C ABI.

The wide kernel is taken when N % 4 == 0, C % 4 == 0, every operand is 16-byte aligned and there is no img_scale; the 32 x 32 dword
kernel keeps the rest.  Both sides of that rule are held to the same checks here:
  out        equals x.permute(0, 2, 1) (+ add_tm), computed by torch in fp32, BIT FOR BIT (a copy, or one correctly rounded add)
  statistics sum g and sum g * yhat of the stored g against fp64 at the `sums` bar of tests/test_hip_dense_fp64.py
             (err <= max(8 * yardstick, 2^-23), the yardstick being tests/dense_ref.py in torch fp32), `sums` zero on entry
  buffers    out and sums written exactly, their guard bands intact
Shapes: a tile is 32 channels x at most 32 float4 of tokens, an image's float4 columns cut into equal tiles.  C: below one float4
(1, 3: the dword kernel), one float4, around one tile (31, 32, 33), a ragged last tile (80), cfg2's 320.  N: one float4 (4), two,
9 (36), 16 and 17 float4 (64, 68), cfg2's 324 (3 tiles of 27), 1 296 (11 tiles of 30, the last one of 24).  Ineligible: N = 1, 49, 81
and views that start 4 bytes off a 16-byte boundary."""
import pytest
import torch

import dense_ref as D
import test_hip_dense_fp64 as T

pytestmark = pytest.mark.gpu

ELIGIBLE = [(B, C, N) for B in (1, 3) for C in (1, 3, 4, 31, 32, 33, 80, 320) for N in (4, 8, 36, 64, 68, 324, 1296)]
INELIGIBLE = [(B, C, N) for B in (1, 3) for C in (4, 33, 320) for N in (1, 49, 81)]


def _case(B, C, N, off=()):
    """Inputs of one case; the operands named in `off` are views that start one float past a 16-byte boundary."""
    gen = torch.Generator(device="cuda").manual_seed(1000 * B + 7 * C + N)
    R = B * N

    def mk(name, *shape, scale=1.0, shift=0.0):
        n = 1
        for s in shape:
            n *= s
        buf = torch.randn(n + 4, device="cuda", generator=gen) * scale + shift
        o = 1 if name in off else 0
        assert (buf.data_ptr() & 15) == 0
        return buf[o:o + n].view(*shape)

    x = mk("x", B, C, N)
    add = mk("add", R, C)
    y = mk("y", R, C, scale=1.5, shift=3.0)                 # pre-BN activations are not centred
    y64 = y.double()
    mean = y64.mean(0)
    invstd = 1.0 / torch.sqrt(((y64 - mean) ** 2).mean(0) + T.EPS)
    return x, add, y, mean.float().contiguous(), invstd.float().contiguous()


def _out(R, C, off):
    full = torch.full((R * C + 2 * T.G + 4,), float("nan"), device="cuda")
    o = 1 if off else 0
    return full, full[T.G + o:T.G + o + R * C]


def _out_ok(full, R, C, off):
    o = 1 if off else 0
    mid = full[T.G + o:T.G + o + R * C]
    return bool(torch.isfinite(mid).all()) and bool(torch.isnan(full[:T.G + o]).all()) and bool(torch.isnan(full[T.G + o + R * C:]).all())


def _check(B, C, N, off=()):
    lib = T._lib()
    from gkgnet_amd import _lib as L
    R = B * N
    x, add, y, mean, invstd = _case(B, C, N, off)
    bars = T.Bars(f"nchw_to_tm_wide B{B} C{C} N{N} off{sorted(off)}")
    want = x.permute(0, 2, 1).reshape(R, C).contiguous()
    want_add = want + add
    oo = "out" in off
    full, o = _out(R, C, oo)
    assert lib.gkg_nchw_to_tm(T._p(x), T._p(o), B, C, N, L.F32, None, T._st()) == 0, lib.gkg_last_error_string()
    torch.cuda.synchronize()
    bars.true("plain: written exactly", _out_ok(full, R, C, oo))
    bars.equal("plain", o.view(R, C), want)
    full, o = _out(R, C, oo)
    assert lib.gkg_nchw_to_tm_add(T._p(x), T._p(add), T._p(o), B, C, N, T._st()) == 0, lib.gkg_last_error_string()
    torch.cuda.synchronize()
    bars.true("add: written exactly", _out_ok(full, R, C, oo))
    bars.equal("add", o.view(R, C), want_add)
    for name, a, g in (("stats + add", add, want_add), ("stats, add_tm NULL", None, want)):
        full, o = _out(R, C, oo)
        sfull = torch.full((2 * C + 16,), 3.0, dtype=torch.float64, device="cuda")
        sums = sfull[8:8 + 2 * C]
        sums.zero_()
        rc = lib.gkg_nchw_to_tm_add_bnstats(T._p(x), T._p(a), T._p(o), T._p(y), T._p(mean), T._p(invstd), T._p(sums), B, C, N, T._st())
        assert rc == 0, lib.gkg_last_error_string()
        torch.cuda.synchronize()
        bars.true(name + ": written exactly", _out_ok(full, R, C, oo))
        bars.true(name + ": sums guards", bool((sfull[:8] == 3.0).all()) and bool((sfull[-8:] == 3.0).all()))
        bars.equal(name, o.view(R, C), g)
        ref, scale = D.bn_bwd_sums(g.double()[None], y.double()[None], mean.double()[None], invstd.double()[None])
        yard, _ = D.bn_bwd_sums(g[None], y[None], mean[None], invstd[None])
        bars.check("sums", name + " fp64 sums", sums.view(1, 2, C), ref, yard, scale)
    bars.done()


@pytest.mark.parametrize("B,C,N", ELIGIBLE)
def test_wide_relayout(B, C, N):
    _check(B, C, N)


@pytest.mark.parametrize("B,C,N", INELIGIBLE)
def test_token_counts_the_wide_form_does_not_take(B, C, N):
    _check(B, C, N)


@pytest.mark.parametrize("off", [("x",), ("out",), ("add",), ("y",), ("x", "out", "add", "y")])
@pytest.mark.parametrize("B,C,N", [(3, 32, 36), (1, 80, 324)])
def test_views_four_bytes_off_alignment(B, C, N, off):
    _check(B, C, N, frozenset(off))
