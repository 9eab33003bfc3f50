"""The tiled derive-apply kernel behind gkg_bn_apply_train / gkg_bn_apply_train_sync (token-major output, csrc/gkg_dense.hip
bn_apply_tiled_kernel) through the C ABI, bit for bit against the two launches it stands for:

    gkg_bn_finalize (a, c, mean, invstd, running statistics from the column sums)  ->  gkg_affine_act (the flat apply kernel)

The column sums are tests/dense_ref.py's fp64 column sums of a random y, rounded to fp32 and widened again: gkg_bn_finalize reads
fp32 sums and widens them, the apply reads fp64 sums, so both derive from the same numbers and every bit must agree (the
arithmetic behind them is the same fp64 chain).  Nothing here needs a tolerance.

Shapes: the edges of a (row chunk) x (channel tile) decomposition whose tile is at most 64 float4 column groups — C = 16 (less than
one tile), 80, 544 (136 column groups: three tiles of 46, 46 and 44, the last one partly idle), 1280 (many tiles); R = 1, 81 (no
multiple of any row-lane count or chunk), 2560; nb = 1 and the grouped layout nb = 4 (group q at column q C of a row of 4 C; with
ochunk, where a group's x | m chunks take 2 C columns, at column 2 q C of a row of 8 C).  Every shape with and without the
residual, act 0 / 1, ochunk 0 / C / 4, and two forms with a row_scale of one factor per 7 rows (7 divides no row chunk and no
row-lane count: a thread's rows in flight straddle factors).  One reference per shape, shared by its ten forms."""
import functools

import pytest
import torch

import dense_ref as D

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
G = 64                                    # guard band, floats
RM0, RV0 = 100.0, 5.0                     # sentinels the running statistics start from (far from any mean + bias)
SHAPES = [(C, nb, R) for C in (16, 80, 544, 1280) for nb in (1, 4) for R in (1, 81, 2560)]
RPS = 7                                   # rows per DropPath factor: divides no row chunk and no row-lane count
FORMS = ([(res, act, och, 0) for res in (False, True) for act in (0, 1) for och in (False, True)]
         + [(True, 1, False, RPS), (False, 0, True, RPS)])


def _lib():
    from gkgnet_amd import _lib
    return _lib.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    from gkgnet_amd.ops import _stream
    return _stream()


def _nan(n):
    full = torch.full((n + 2 * G,), float("nan"), device="cuda")
    return full, full[G:G + n]


def _bits(t):
    return t.view(torch.int32)


@functools.lru_cache(maxsize=2)
def _case(C, nb, R, count):
    """Inputs of one shape, the sums both paths derive from, and what gkg_bn_finalize makes of them (`count` rows)."""
    lib = _lib()
    gen = torch.Generator(device="cuda").manual_seed(1000 * C + 10 * R + nb)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)      # noqa: E731
    u = lambda *s: torch.rand(*s, device="cuda", generator=gen)       # noqa: E731
    std = u(nb, 1, C) + 0.5
    y = (r(nb, R, C) * std + (u(nb, 1, C) - 0.5) * 4.0 * std).contiguous()
    k = dict(y=y, res=r(nb, R, C), gamma=u(nb, C) + 0.5, beta=r(nb, C), bias=r(nb, C), row_scale=u(-(-R // RPS)) * 1.5 + 0.25)
    # the sums of `count` rows with y's column means (count == R: y's own sums)
    sums32 = (D.col_sums(y.double()) * (count / R)).float().contiguous()
    k["sums32"], k["sums64"] = sums32, sums32.double().contiguous()
    fin = {n: torch.full((nb, C), float("nan"), device="cuda") for n in ("a", "c", "mean", "invstd")}
    fin["rm"], fin["rv"] = torch.full((nb, C), RM0, device="cuda"), torch.full((nb, C), RV0, device="cuda")
    cnt = torch.tensor([float(count)], device="cuda")
    rc = lib.gkg_bn_finalize(_p(sums32), _p(cnt), _p(k["gamma"]), _p(k["beta"]), _p(k["bias"]), _p(fin["rm"]), _p(fin["rv"]),
                             *[_p(fin[n]) for n in ("a", "c", "mean", "invstd")], C, nb, MOM, EPS, None, _st())
    assert rc == 0, lib.gkg_last_error_string()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in fin.values())
    k["fin"] = fin
    return k


def _layout(C, nb, R, och):
    """(ldo, out_bstride, ochunk, elements of the output buffer)."""
    if nb == 1:
        ldo, bstride = (2 * C if och else C + 8), 0
    else:
        ldo, bstride = (8 * C, 2 * C) if och else (4 * C, C)
    return ldo, bstride, (C // 4 if och else 0), R * ldo


def _written(nb, R, C, ldo, bstride, ochunk, n):
    cols = D.xm_cols(C, ochunk, "cuda")
    idx = (torch.arange(nb, device="cuda")[:, None, None] * bstride + torch.arange(R, device="cuda")[None, :, None] * ldo + cols[None, None, :])
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask[idx.reshape(-1)] = True
    assert int(mask.sum()) == nb * R * C                               # the layout itself writes no element twice
    return mask


def _run(C, nb, R, count, sync):
    lib = _lib()
    k = _case(C, nb, R, count)
    fin = k["fin"]
    bad = []
    cnt64 = torch.tensor([float(count)], dtype=torch.float64, device="cuda")
    for res, act, och, rps in FORMS:
        tag = f"res{int(res)} act{act} och{int(och)} rps{rps}"
        rs = k["row_scale"] if rps else None
        ldo, bstride, ochunk, n = _layout(C, nb, R, och)
        mask = _written(nb, R, C, ldo, bstride, ochunk, n)
        sv = {nm: _nan(nb * C) for nm in ("a", "c", "mean", "invstd")}
        rm, rv = torch.full((nb, C), RM0, device="cuda"), torch.full((nb, C), RV0, device="cuda")
        nbt = torch.tensor([41], dtype=torch.int64, device="cuda")
        zd = 2 * nb * C + 7                                            # odd
        zfull = torch.full((zd + 16,), 3.0, dtype=torch.float64, device="cuda")
        cout_full, cout = _nan(1)
        full, o = _nan(n)
        args = [_p(k["y"]), _p(k["sums64"]), _p(k["gamma"]), _p(k["beta"]), _p(k["bias"]), _p(rm), _p(rv), _p(nbt),
                *[_p(sv[nm][1]) for nm in ("a", "c", "mean", "invstd")], _p(k["res"]) if res else None, _p(o), R, C, nb, ldo, bstride,
                ochunk, act, 0, _p(rs), rps, MOM, EPS, _p(zfull[8:]), zd]
        if sync:
            rc = lib.gkg_bn_apply_train_sync(*args, _p(cnt64), _p(cout), _st())
        else:
            rc = lib.gkg_bn_apply_train(*args, _st())
        assert rc == 0, lib.gkg_last_error_string()
        full2, o2 = _nan(n)
        rc = lib.gkg_affine_act(_p(k["y"]), _p(sv["a"][1]), _p(sv["c"][1]), _p(k["res"]) if res else None, _p(o2), R, C, nb, ldo, bstride,
                                ochunk, act, 0, _p(rs), rps, _st())
        assert rc == 0, lib.gkg_last_error_string()
        torch.cuda.synchronize()
        mid = full[G:G + n]
        if not (bool(torch.isfinite(mid[mask]).all()) and bool(torch.isnan(mid[~mask]).all()) and bool(torch.isnan(full[:G]).all())
                and bool(torch.isnan(full[G + n:]).all())):
            bad.append((tag, "out not written exactly"))
        if not torch.equal(_bits(full), _bits(full2)):
            bad.append((tag, "out != gkg_affine_act(saved a, c)", int((_bits(full) != _bits(full2)).sum())))
        for nm in ("a", "c", "mean", "invstd"):
            f, v = sv[nm]
            if not (bool(torch.isnan(f[:G]).all()) and bool(torch.isnan(f[G + nb * C:]).all())):
                bad.append((tag, nm + " guards"))
            if not torch.equal(_bits(v.view(nb, C)), _bits(fin[nm])):
                bad.append((tag, nm + " != gkg_bn_finalize", int((_bits(v.view(nb, C)) != _bits(fin[nm])).sum())))
        # every channel of every group exactly once: ONE momentum step from the sentinel, the bits of gkg_bn_finalize's step
        for nm, got, start in (("running_mean", rm, RM0), ("running_var", rv, RV0)):
            want = fin["rm" if nm == "running_mean" else "rv"]
            if not torch.equal(_bits(got), _bits(want)):
                bad.append((tag, nm + " != gkg_bn_finalize", int((_bits(got) != _bits(want)).sum())))
        one = (1.0 - MOM) * RM0 + MOM * (fin["mean"].double() + k["bias"].double())
        two = (1.0 - MOM) * one + MOM * (fin["mean"].double() + k["bias"].double())
        if not bool(((rm.double() - one).abs() <= 1e-5 * (one.abs() + 1.0)).all()):
            bad.append((tag, "running_mean is not one momentum step from the sentinel"))
        if not bool(((rm.double() - two).abs() > 1e-3).all()):          # |one - two| = MOM (1 - MOM) |RM0 - mean - bias| > 8
            bad.append((tag, "running_mean took a second step somewhere"))
        if int(nbt) != 42:
            bad.append((tag, "num_batches_tracked", int(nbt)))
        if not (bool((zfull[8:8 + zd] == 0).all()) and bool((zfull[:8] == 3.0).all()) and bool((zfull[8 + zd:] == 3.0).all())):
            bad.append((tag, "zero_buf"))
        if sync and not (float(cout) == float(count) and bool(torch.isnan(cout_full[:G]).all()) and bool(torch.isnan(cout_full[G + 1:]).all())):
            bad.append((tag, "count_out", float(cout)))
        if not sync and not bool(torch.isnan(cout_full).all()):
            bad.append((tag, "count_out touched"))
    assert not bad, (C, nb, R, bad)


@pytest.mark.parametrize("C,nb,R", SHAPES)
def test_bn_apply_train_tiled_bits(C, nb, R):
    """out == gkg_affine_act with the a, c the call saved; a, c, mean, invstd, running statistics == gkg_bn_finalize's from the same
    sums; num_batches_tracked + 1; an odd number of zero_buf doubles cleared and nothing beyond; one momentum step per channel."""
    _run(C, nb, R, R, sync=False)


@pytest.mark.parametrize("C,nb,R", SHAPES)
def test_bn_apply_train_sync_tiled_bits(C, nb, R):
    """The same comparison for gkg_bn_apply_train_sync with a device `count` that is not R (3 R + 5 rows over all ranks): the
    statistics are gkg_bn_finalize's for that count, count_out receives it as fp32."""
    _run(C, nb, R, 3 * R + 5, sync=True)
