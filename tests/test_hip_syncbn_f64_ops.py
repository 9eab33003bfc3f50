"""The fp64 SyncBatchNorm halves of csrc/gkg_dense.hip / gkg_knn.hip through the C ABI: gkg_bn_apply_train_sync, _dual_sync,
gkg_bn_apply_knn_prep_sync, gkg_bn_bwd_stats_f64 and gkg_bn_bwd_apply_sync.

Method, classes, K factors and FLOOR are those of tests/test_hip_dense_fp64.py (imported, see THE BAR there): fp64 reference from
tests/dense_ref.py, the same formula in torch fp32 as the yardstick, NaN-prefilled outputs between guard bands, sentinel bands
round zero_buf.  Ranks are simulated by row parts of ONE matrix: every part's column sums are taken in torch fp64 from its fp32 y,
the parts are added (the "all-reduce"), the count is the total number of rows, and every part is run through the kernel on its own.
The parts are unequal on purpose: a kernel that divides by its own R instead of the exchanged count fails every check below.

The derive is fp64 from the sums to the fp32 store, so the |mean| = 1e4 std case is held to the same bar as every other (the fp32
plain-sums halves gkg_bn_stats_sums / gkg_bn_finalize are exempted there in test_hip_dense_fp64.py)."""
import pytest
import torch

import dense_ref as D
import test_hip_dense_fp64 as F
from test_hip_dense_fp64 import (EPS, MOM, Bars, _cleared_exactly, _dd, _guards_intact, _inputs, _lib, _nan, _p, _param_checks, _rel,
                                 _sentinel_doubles, _st, _tm_mask, _written_exactly)

pytestmark = pytest.mark.gpu

ERR_NULL, ERR_SHAPE = F.ERR_NULL, F.ERR_SHAPE
PARTS = [(1, 15), (17, 255), (72, 128)]
CS = [4, 36, 68, 320]


def _bounds(parts):
    out, r0 = [], 0
    for n in parts:
        out.append((r0, r0 + n))
        r0 += n
    return out


def _exchange(y, parts):
    """-> (the all-reduced buffer [nb][2][C] sums + [count], fp64): per-part fp64 sums of the fp32 y, added over the parts."""
    tot = sum(D.col_sums(y[:, r0:r1].double()) for r0, r1 in _bounds(parts))
    return torch.cat([tot.reshape(-1), torch.tensor([float(y.shape[1])], dtype=torch.float64, device="cuda")]).contiguous()


class _Fwd:
    """What every forward case shares: inputs, the exchanged buffer, the reference statistics of the concatenated matrix."""

    def __init__(self, parts, C, nb, seed, offset=3.0):
        self.parts, self.C, self.nb, self.R = parts, C, nb, sum(parts)
        self.k = _inputs(nb, self.R, C, seed, offset)
        self.buf = _exchange(self.k["y"], parts)
        self.count_ptr = self.buf.data_ptr() + 8 * 2 * nb * C
        self.st64 = D.bn_stats(*_dd(self.k, "y", "gamma", "beta"), EPS)
        self.st32 = D.bn_stats(self.k["y"], self.k["gamma"], self.k["beta"], EPS)

    def head(self):
        """Fresh per-"rank" parameter outputs, running statistics, count_out and zero_buf -> (argument head, state)."""
        nb, C, k = self.nb, self.C, self.k
        s = dict(out_p={n: _nan(nb * C) for n in ("a", "c", "mean", "invstd")}, rm=k["rm"].clone(), rv=k["rv"].clone(),
                 nbt=torch.tensor([41], dtype=torch.int64, device="cuda"), cnt=_nan(1), zd=2 * nb * C + 7)
        s["zfull"], s["z"] = _sentinel_doubles(s["zd"])
        head = (_p(self.buf), _p(k["gamma"]), _p(k["beta"]), _p(k["bias"]), _p(s["rm"]), _p(s["rv"]), _p(s["nbt"]),
                *[_p(s["out_p"][n][1]) for n in ("a", "c", "mean", "invstd")])
        return head, s

    def check_side(self, bars, s, tag):
        nb, C = self.nb, self.C
        bars.true(tag + " zero_buf cleared, nothing beyond", _cleared_exactly(s["zfull"], s["zd"]))
        bars.true(tag + " param guards", all(_guards_intact(f) for f, _ in s["out_p"].values()))
        bars.true(tag + " num_batches_tracked", int(s["nbt"]) == 42)
        bars.true(tag + " count_out", _guards_intact(s["cnt"][0]) and float(s["cnt"][1][0]) == float(self.R))
        got = dict({n: v.view(nb, C) for n, (_, v) in s["out_p"].items()}, rm=s["rm"], rv=s["rv"])
        bars.case, case = bars.case + " " + tag, bars.case
        _param_checks(bars, self.R, self.k, got, self.st64, self.st32, count=float(self.R))      # unbiased with the GLOBAL count
        bars.case = case


def _tm_forms(C):
    forms = [("tm", 0, False), ("tm", 1, True), ("tm", 1, False), ("tm", 0, True)]
    if C % 16 == 0:
        forms += [("ochunk", 0, False), ("ochunk", 1, True)]
    return forms


def _run_tm(parts, C, nb, offset, forms):
    lib = _lib()
    f = _Fwd(parts, C, nb, 31 * sum(parts) + C + nb, offset)
    k = f.k
    bars = Bars(f"apply_train_sync parts{parts} C{C} nb{nb} off{offset:g}")
    for form, act, with_res in forms:
        ochunk = C // 4 if form == "ochunk" else 0
        ldo = 2 * C if ochunk else C + 8
        for (r0, r1) in _bounds(parts):
            Rp = r1 - r0
            tag = f"{form} act{act} res{int(with_res)} rows[{r0},{r1})"
            y = k["y"][:, r0:r1].contiguous()
            res = k["res"][:, r0:r1].contiguous() if with_res else None
            bstride = Rp * ldo + 12
            n = nb * bstride
            full, o = _nan(n)
            head, s = f.head()
            rc = lib.gkg_bn_apply_train_sync(_p(y), *head, _p(res), _p(o), Rp, C, nb, ldo, bstride, ochunk, act, 0, None, 0, MOM, EPS,
                                             _p(s["z"]), s["zd"], f.count_ptr, _p(s["cnt"][1]), _st())
            assert rc == 0, lib.gkg_last_error_string()
            torch.cuda.synchronize()
            mask, idx = _tm_mask(nb, Rp, C, ldo, bstride, ochunk, n)
            bars.true(tag + " out written exactly", _written_exactly(full, mask))
            ref, scale = D.affine_act(y.double(), f.st64["a"], f.st64["c"], act, None, 1, None if res is None else res.double())
            yard, _ = D.affine_act(y, f.st32["a"], f.st32["c"], act, None, 1, res)
            bars.check("fwd", tag + " out", o[idx], ref, yard, scale)
            f.check_side(bars, s, tag)
    bars.done()


@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("parts", PARTS)
def test_apply_train_sync_token_major(parts, C, nb):
    _run_tm(parts, C, nb, 3, _tm_forms(C))


def test_apply_train_sync_mean_1e4_std():
    """E[y^2] - E[y]^2 of fp64 sums of fp32 values: 1e8 below the squares, 1e-8 of the variance left of fp64's 1e-16 — the same bar."""
    _run_tm((72, 128), 68, 1, 1e4, [("tm", 1, True), ("tm", 0, False)])


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("C", CS)
def test_apply_train_sync_channel_major(C, with_res):
    lib = _lib()
    N, imgs = 25, (1, 2)
    f = _Fwd(tuple(b * N for b in imgs), C, 1, 37 * C + int(with_res))
    k = f.k
    bars = Bars(f"apply_train_sync nchw imgs{imgs} N{N} C{C} res{int(with_res)}")
    for Bp, (r0, r1) in zip(imgs, _bounds(f.parts)):
        tag = f"images{Bp}"
        y = k["y"][0, r0:r1].contiguous()
        res = k["res"][0, r0:r1].view(Bp, N, C).permute(0, 2, 1).contiguous() if with_res else None
        full, o = _nan(Bp * N * C)
        head, s = f.head()
        rc = lib.gkg_bn_apply_train_sync(_p(y), *head, _p(res), _p(o), Bp * N, C, 1, C, 0, 0, 0, Bp, None, N, MOM, EPS, _p(s["z"]), s["zd"],
                                         f.count_ptr, _p(s["cnt"][1]), _st())
        assert rc == 0, lib.gkg_last_error_string()
        torch.cuda.synchronize()
        bars.true(tag + " out written exactly", _written_exactly(full, torch.ones(Bp * N * C, dtype=torch.bool, device="cuda")))
        ref, scale = D.tm_affine_to_nchw(y.double(), Bp, C, N, f.st64["a"][0], f.st64["c"][0], None if res is None else res.double())
        yard, _ = D.tm_affine_to_nchw(y, Bp, C, N, f.st32["a"][0], f.st32["c"][0], res)
        bars.check("fwd", tag + " out", o, ref, yard, scale)
        f.check_side(bars, s, tag)
    bars.done()


# ------------------------------------------------------------------------------------------------------------------ dual / knn-prep
def _vs_local(bars, tag, got, local, yard, scale):
    """The _sync form on a part against its LOCAL sibling run on the concatenated batch (the reference here), same bar: the
    yardstick is the plain-torch fp32 formula's distance from that reference."""
    bars.check("fwd", tag, got, local.double(), yard, scale)


def test_apply_train_dual_sync_equals_the_local_kernel_on_the_whole_batch():
    """Shapes of tests/test_hip_dual_layout.py (B = 4, C = 64, 12 x 12 tokens), split 1 + 3 images."""
    lib = _lib()
    B, C, N, imgs = 4, 64, 144, (1, 3)
    f = _Fwd(tuple(b * N for b in imgs), C, 1, 4101)
    k = f.k
    bars = Bars("apply_train_dual_sync B4 C64 N144 imgs(1,3)")
    y, res_tm = k["y"][0], k["res"][0]
    head, s0 = f.head()
    o_full, otm_full = torch.empty(B * C * N, device="cuda"), torch.empty(B * N * C, device="cuda")
    rc = lib.gkg_bn_apply_train_dual(_p(y), *head, _p(res_tm), _p(o_full), _p(otm_full), B, C, N, MOM, EPS, _p(s0["z"]), s0["zd"], _st())
    assert rc == 0, lib.gkg_last_error_string()
    _, yard_tm, scale = D.tm_affine_to_nchw_dual(y, B, C, N, f.st32["a"][0], f.st32["c"][0], res_tm)
    for Bp, (r0, r1) in zip(imgs, _bounds(f.parts)):
        tag = f"images{Bp}"
        full, o = _nan(Bp * C * N)
        ftm, otm = _nan(Bp * N * C)
        head, s = f.head()
        yp, rp = y[r0:r1].contiguous(), res_tm[r0:r1].contiguous()
        rc = lib.gkg_bn_apply_train_dual_sync(_p(yp), *head, _p(rp), _p(o), _p(otm), Bp, C, N, MOM, EPS, _p(s["z"]), s["zd"], f.count_ptr,
                                              _p(s["cnt"][1]), _st())
        assert rc == 0, lib.gkg_last_error_string()
        torch.cuda.synchronize()
        every = torch.ones(Bp * N * C, dtype=torch.bool, device="cuda")
        bars.true(tag + " written exactly", _written_exactly(full, every) and _written_exactly(ftm, every))
        _vs_local(bars, tag + " out_tm", otm.view(r1 - r0, C), otm_full.view(B * N, C)[r0:r1], yard_tm[r0:r1], scale[r0:r1])
        bars.equal(tag + " out == out_tm transposed", o.view(Bp, C, N), otm.view(Bp, N, C).permute(0, 2, 1).contiguous())
        f.check_side(bars, s, tag)
    bars.done()


def test_apply_knn_prep_sync_equals_the_local_kernel_on_the_whole_batch():
    """A shape of tests/test_hip_knn_prep_fused.py (B = 5, G = 4, c = 20, N = 200, k = 5, self graph, plain rows), split 2 + 3 images:
    x, the saved statistics and — through the k-NN call that follows with GKG_KNN_X_PREPARED — the prepared tokens."""
    from gkgnet_amd import _lib as L
    lib = _lib()
    B, G, c, N, kk, d, imgs = 5, 4, 20, 200, 5, 1, (2, 3)
    C = G * c
    f = _Fwd(tuple(b * N for b in imgs), C, 1, 7 * N + c)
    k = f.k
    bars = Bars("apply_knn_prep_sync B5 G4 c20 N200 imgs(2,3)")
    flags = L.KNN_NORMALIZE
    y = k["y"][0]

    def run(yp, Bp, sync):
        wsb = lib.gkg_knn_workspace_bytes(Bp * G, c, N, N, kk, d, L.F32, L.KNN_NORMALIZE)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        full, out = _nan(Bp * N * C)
        head, s = f.head()
        args = (_p(yp), *head, _p(out), C, 0, Bp, G, c, N, N, kk, d, 0, 0, flags, 0, 0, None, None, _p(ws), wsb, MOM, EPS, _p(s["z"]), s["zd"])
        if sync:
            rc = lib.gkg_bn_apply_knn_prep_sync(*args, f.count_ptr, _p(s["cnt"][1]), _st())
        else:
            rc = lib.gkg_bn_apply_knn_prep(*args, _st())
        assert rc == 0, lib.gkg_last_error_string()
        nn16 = torch.empty((Bp * G, N, kk), dtype=torch.int16, device="cuda")
        rc = lib.gkg_knn_fwd_tm16(_p(out), C, 0, None, None, _p(nn16), Bp, G, c, N, N, kk, d, L.F32, flags | L.KNN_X_PREPARED, _p(ws), wsb, _st())
        assert rc == 0, lib.gkg_last_error_string()
        torch.cuda.synchronize()
        return full, out, s, nn16

    _, out0, s0, nn0 = run(y.contiguous(), B, False)
    yard, scale = D.affine_act(k["y"], f.st32["a"], f.st32["c"])
    b0 = 0
    for Bp, (r0, r1) in zip(imgs, _bounds(f.parts)):
        tag = f"images{Bp}"
        full, out, s, nn = run(y[r0:r1].contiguous(), Bp, True)
        bars.true(tag + " out written exactly", _written_exactly(full, torch.ones(Bp * N * C, dtype=torch.bool, device="cuda")))
        _vs_local(bars, tag + " x", out.view(r1 - r0, C), out0.view(B * N, C)[r0:r1], yard[0, r0:r1], scale[0, r0:r1])
        bars.equal(tag + " graphs of these images", nn, nn0[b0 * G:(b0 + Bp) * G])
        b0 += Bp
        f.check_side(bars, s, tag)
    bars.done()


# ------------------------------------------------------------------------------------------------------------------ backward
# (parts, C, nb, dout layout, rows_per_scale): every part / C pair of the forward cases, nb 1 and 4 alternating; one wide-ldg layout
# and one row-scale case (8 divides 72 and 128: the concatenated scale vector describes the whole batch with the same rows_per_scale)
BWD = [(p, C, (1, 4)[(i + j) % 2], "padded", 0) for i, p in enumerate(PARTS) for j, C in enumerate(CS)]
BWD += [((17, 255), 68, 4, "wide", 0), ((72, 128), 36, 2, "padded", 8)]


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("parts,C,nb,layout,rps", BWD)
def test_bn_backward_sync(parts, C, nb, layout, rps, act):
    lib = _lib()
    R = sum(parts)
    k = _inputs(nb, R, C, 41 * R + C + nb + act)
    sv = F._saved(k, R)                                          # the statistics of the CONCATENATED matrix, as every rank holds them
    bars = Bars(f"bn_bwd_sync parts{parts} C{C} nb{nb} act{act} {layout} rps{rps}")
    dd = lambda t: t.double()      # noqa: E731
    rs_parts = [None if not rps else torch.rand(n // rps, device="cuda", generator=k["gen"]) * 1.5 + 0.25 for n in parts]
    rs = torch.cat(rs_parts) if rps else None
    stat = (sv["a"], sv["c"], sv["mean"], sv["invstd"])
    ref = D.bn_bwd(dd(k["dout"]), dd(k["y"]), *[dd(t) for t in stat], act, None if rs is None else dd(rs), rps or 1)
    yard = D.bn_bwd(k["dout"], k["y"], *stat, act, rs, rps or 1)
    ranks = []
    for (r0, r1), rsp in zip(_bounds(parts), rs_parts):
        Rp = r1 - r0
        tag = f"rows[{r0},{r1})"
        y, dout = k["y"][:, r0:r1].contiguous(), k["dout"][:, r0:r1].contiguous()
        holder, gptr, ldg, gbs = F._dout_layout(dict(dout=dout, gen=k["gen"]), nb, Rp, C, layout == "wide")
        before = holder.clone()
        sfull = torch.full((2 * nb * C + 16,), 3.0, dtype=torch.float64, device="cuda")
        sums = sfull[8:8 + 2 * nb * C]
        sums.zero_()
        args = (_p(gptr), _p(y), *[_p(t) for t in stat])
        rc = lib.gkg_bn_bwd_stats_f64(*args, Rp, C, nb, ldg, gbs, act, _p(sums), _p(rsp), rps, _st())
        assert rc == 0, lib.gkg_last_error_string()
        torch.cuda.synchronize()
        bars.true(tag + " sums guards", bool((sfull[:8] == 3.0).all()) and bool((sfull[-8:] == 3.0).all()))
        bars.equal(tag + " dout not modified by the statistics half", holder, before)
        dz64 = D.bn_bwd_dz(dd(dout), dd(y), dd(sv["a"]), dd(sv["c"]), act, None if rsp is None else dd(rsp), rps or 1)
        dz32 = D.bn_bwd_dz(dout, y, sv["a"], sv["c"], act, rsp, rps or 1)
        s64, abs64 = D.bn_bwd_sums(dz64, dd(y), dd(sv["mean"]), dd(sv["invstd"]))
        s32, _ = D.bn_bwd_sums(dz32, y, sv["mean"], sv["invstd"])
        bars.check("sums", tag + " fp64 sums", sums.view(nb, 2, C), s64, s32, abs64)
        ranks.append(dict(tag=tag, r=(r0, r1), y=y, holder=holder, before=before, args=args, ldg=ldg, gbs=gbs, local=sums.clone(), rsp=rsp,
                          s64=s64, s32=s32, abs64=abs64))
    total = sum(r["local"] for r in ranks).contiguous()           # the "all-reduce"
    count = torch.tensor([float(R)], device="cuda")
    for r in ranks:
        (r0, r1), tag = r["r"], r["tag"]
        Rp = r1 - r0
        fdy, dy = _nan(nb * Rp * C)
        fdg, dg = _nan(nb * C)
        fdb, db = _nan(nb * C)
        zd = 2 * nb * C + 2
        zfull, zb = _sentinel_doubles(zd)
        rc = lib.gkg_bn_bwd_apply_sync(*r["args"], _p(dy), _p(dg), _p(db), Rp, C, nb, r["ldg"], r["gbs"], act, _p(r["local"]), _p(total),
                                       _p(count), _p(zb), zd, _p(r["rsp"]), rps, _st())
        assert rc == 0, lib.gkg_last_error_string()
        torch.cuda.synchronize()
        bars.true(tag + " dy written exactly", _written_exactly(fdy, torch.ones(nb * Rp * C, dtype=torch.bool, device="cuda")))
        bars.true(tag + " dgamma / dbeta guards", _guards_intact(fdg) and _guards_intact(fdb))
        bars.true(tag + " zero_buf cleared, nothing beyond", _cleared_exactly(zfull, zd))
        bars.equal(tag + " dout not modified", r["holder"], r["before"])
        # dy: this part's rows of the full-batch backward
        bars.check("dy", tag + " dy", dy, ref["dy"][:, r0:r1], yard["dy"][:, r0:r1], ref["dy_scale"][:, r0:r1])
        # dgamma / dbeta: the part's OWN sums (the data-parallel gradient exchange adds them up), not the exchanged ones
        bars.check("param", tag + " dbeta", db, r["s64"][:, 0], r["s32"][:, 0], r["abs64"][:, 0])
        bars.check("param", tag + " dgamma", dg, r["s64"][:, 1], r["s32"][:, 1], r["abs64"][:, 1])
        far = _rel(dg.view(nb, C), ref["sums"][:, 1], r["abs64"][:, 1])
        bars.true(tag + f" dgamma is not the global sum (distance {far:.3g})", far > 1e-3)
    bars.done()


# ------------------------------------------------------------------------------------------------------------------ rejections
def _sync_reject_calls(lib):
    from gkgnet_amd import _lib as L
    R, Cn = 16, 8
    big = R * Cn * 65 + 64
    outs = [torch.full((big,), float("nan"), device="cuda") for _ in range(9)]
    o = [t.data_ptr() for t in outs]
    src = torch.ones(big, device="cuda")
    dsrc = torch.zeros(2 * Cn * 65 + 2, dtype=torch.float64, device="cuda")
    dsrc[-1] = float(R)
    s, d = src.data_ptr(), dsrc.data_ptr()
    cnt64 = d + 8 * (2 * Cn * 65 + 1)
    cnt32 = torch.tensor([float(R)], device="cuda")
    wsb = lib.gkg_knn_workspace_bytes(1 * 2, 4, R, R, 3, 1, L.F32, L.KNN_NORMALIZE)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")

    def run(nb=2, null_count=False, zero_no_buf=False, single=False):
        rm, rv = (s, None) if single else (o[5], o[6])
        c64, c32 = (None, None) if null_count else (cnt64, cnt32.data_ptr())
        zd = 4 if zero_no_buf else 0
        return dict(
            apply_train_sync=lambda: lib.gkg_bn_apply_train_sync(s, d, s, s, s, rm, rv, None, o[0], o[1], o[2], o[3], None, o[4], R, Cn, nb, Cn,
                                                                 R * Cn, 0, 1, 0, None, 0, MOM, EPS, None, zd, c64, o[7], None),
            apply_train_dual_sync=lambda: lib.gkg_bn_apply_train_dual_sync(s, d, s, s, s, rm, rv, None, o[0], o[1], o[2], o[3], s, o[4], o[8],
                                                                           1, Cn, R, MOM, EPS, None, zd, c64, o[7], None),
            apply_knn_prep_sync=lambda: lib.gkg_bn_apply_knn_prep_sync(s, d, s, s, s, rm, rv, None, o[0], o[1], o[2], o[3], o[4], Cn, 0, 1, 2, 4,
                                                                       R, R, 3, 1, 0, 0, L.KNN_NORMALIZE, 0, 0, None, None, ws.data_ptr(),
                                                                       ws.numel(), MOM, EPS, None, zd, c64, o[7], None),
            bwd_stats_f64=lambda: lib.gkg_bn_bwd_stats_f64(s, s, s, s, s, s, R, Cn, nb, Cn, R * Cn, 1, d, None, 0, None),
            bwd_apply_sync=lambda: lib.gkg_bn_bwd_apply_sync(s, s, s, s, s, s, o[0], o[1], o[2], R, Cn, nb, Cn, R * Cn, 1, d, d, c32, None, zd,
                                                             None, 0, None),
        )
    return run, outs, dsrc


SYNC_REJECT = {
    "null count": (dict(null_count=True), ERR_NULL, ("apply_train_sync", "apply_train_dual_sync", "apply_knn_prep_sync", "bwd_apply_sync")),
    "nb > 64": (dict(nb=65), ERR_SHAPE, ("apply_train_sync", "bwd_stats_f64", "bwd_apply_sync")),
    "zero_doubles without zero_buf": (dict(zero_no_buf=True), ERR_SHAPE, ("apply_train_sync", "apply_train_dual_sync", "apply_knn_prep_sync",
                                                                          "bwd_apply_sync")),
    "running statistics given singly": (dict(single=True), ERR_NULL, ("apply_train_sync", "apply_train_dual_sync", "apply_knn_prep_sync")),
}


@pytest.mark.parametrize("what", list(SYNC_REJECT))
def test_sync_bad_arguments_are_rejected_and_nothing_is_launched(what):
    lib = _lib()
    run, outs, dsrc = _sync_reject_calls(lib)
    before = dsrc.clone()
    kw, code, names = SYNC_REJECT[what]
    good, bad = run(), run(**kw)
    for name in names:
        rc = bad[name]()
        assert rc == code, (what, name, rc, lib.gkg_last_error_string())
        assert lib.gkg_last_error_string(), name
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs), what                 # nothing ran: every output still holds its NaN fill
    assert torch.equal(dsrc, before), what                                     # ... and the statistics half added nothing to its sums
    for name in names:                                                         # the same calls with good arguments are accepted
        assert good[name]() == 0, (what, name, lib.gkg_last_error_string())
    torch.cuda.synchronize()
