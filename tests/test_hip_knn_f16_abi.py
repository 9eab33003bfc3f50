"""The fp16-contraction k-NN (GKG_KNN_F16_CONTRACT: csrc/gkg_knn_hf.hip, knn_tile_kernel<..., BF = KNN_EL_F16>) through the C ABI,
against the fp64 evaluation of its definition in tests/knn_f16_ref.py (definition, flush, bound E: that module's docstring).  The
sibling of tests/test_hip_knn_bf16_abi.py (``A``): the same forms (``R.FORMS``, described there), the same inputs (``A._case``: one set
of device tensors for both files), the same call between guard bands (``A.call``), with the fp16 flag and the fp16 reference.

A graph that is judged: every index in [0, M), the k entries of a row distinct, at every kept rank the definition distance of the
returned key within 2 E of the reference's, and the share of positions that differ from the reference ranking at most the case's
near-tie share (<= 5 %: tests/test_knn_f16_reference_host.py).  Each case prints its mismatch share and its largest tolerated
gap / 2E under ``pytest -s`` (figures: EXPERIMENTS.md "fp16-contraction k-NN")."""
import functools

import numpy as np
import pytest
import torch

import knn_bf16_ref as R
import knn_f16_ref as H
import test_hip_knn_bf16_abi as A
from util import Buf, xm_pack

pytestmark = pytest.mark.gpu

SELECT = A.SELECT
_K, _p, _st, _dev, _dims, call = A._K, A._p, A._st, A._dev, A._dims, A.call


def _flags(select="auto", f16=True, bf16=False, normalize=True):
    return A._flags(select, normalize=normalize, bf16=bf16) | (_K("KNN_F16_CONTRACT") if f16 else 0)


@functools.lru_cache(maxsize=None)
def _graph(shape):
    """The fp16-contraction graph of a FORMS shape by the library's own rule (token-major entry, int64 lists)."""
    case = A._case(shape)
    return call(_dims(shape), case["x_tm"], case["y_tm"], case["rp_dev"], _flags("auto"))


def judged(got, x, y, rp, c, k, d, what, rows=None):
    """Reference, bound and judge for one graph; asserts the mismatch share against the near-tie share of the judged rows and prints
    the case's figures.  x, y, rp: numpy, channel-major.  -> (D, topd, topi)."""
    D, topd, topi = H.reference(x, y, rp, k, d, device="cuda")
    E = H.bound(c, rp)
    near = H.near_tie_share(topd if rows is None else topd[rows.to(topd.device)], E, k, d)
    share, worst = H.judge(got, D, topd, topi, k, d, E, rows=rows, what=what)
    print(f"knn_f16 {what}: mismatch {100 * share:.4f} % (near ties {100 * near:.3f} %), worst gap/2E {worst:.3f}")
    assert share <= near, f"{what}: mismatch share {share:.5f} above the near-tie share {near:.5f}"
    return D, topd, topi


# ------------------------------------------------------------------------------------------------------------------ (a) definition
@pytest.mark.parametrize("shape", R.FORMS, ids=R.shape_id)
def test_every_form_computes_the_definition(shape):
    B, G, c, N, M_, k, d, bias = shape
    case = A._case(shape)
    got = _graph(shape)
    _, topd, _ = judged(got, case["x"], case["y"], case["rp"], c, k, d, R.shape_id(shape))
    assert H.near_tie_share(topd, H.bound(c, case["rp"]), k, d) <= R.NEAR_TIE_CAP
    for select in ("direct", "buffered"):
        other = call(_dims(shape), case["x_tm"], case["y_tm"], case["rp_dev"], _flags(select))
        assert torch.equal(other, got), f"{R.shape_id(shape)}: the {select} selection differs from the rule's at {int((other != got).sum())} positions"


# ------------------------------------------------------------------------------------------------------------------ (b) entry points
@pytest.mark.parametrize("shape", R.FORMS, ids=R.shape_id)
def test_entry_points_and_list_formats_agree(shape):
    """Channel-major gkg_knn_fwd, the u16 lists of gkg_knn_fwd_tm16 and a call without a centre plane give the token-major graph."""
    case, got, dims = A._case(shape), _graph(shape), _dims(shape)
    cm = call(dims, _dev(case["x"]), _dev(case["y"]), case["rp_dev"], _flags(), entry="cm")
    assert torch.equal(cm, got), "channel-major entry"
    u16 = call(dims, case["x_tm"], case["y_tm"], case["rp_dev"], _flags(), entry="tm16")
    assert torch.equal(u16, got), "u16 lists"
    bare = call(dims, case["x_tm"], case["y_tm"], case["rp_dev"], _flags(), center=False)
    assert torch.equal(bare, got), "center == NULL"


@pytest.mark.parametrize("shape", [R.FORMS[i] for i in (1, 6, 9, 10)], ids=R.shape_id)
def test_x_as_the_x_half_of_an_xm_buffer(shape):
    """x passed as a view (ldx = 2 C, xchunk = C / 4: include/gkg_hip.h "XM layout"); the m half holds NaN."""
    case, got, dims = A._case(shape), _graph(shape), _dims(shape)
    B, G, c, N = dims[:4]
    C = G * c
    assert C % 16 == 0 and c % 4 == 0
    x2 = case["x_tm"].reshape(B * N, C)
    XM = xm_pack(x2, torch.full_like(x2, float("nan"))).contiguous()
    view = call(dims, XM, case["y_tm"], case["rp_dev"], _flags(), ldx=2 * C, xchunk=C // 4)
    assert torch.equal(view, got)
    view16 = call(dims, XM, case["y_tm"], case["rp_dev"], _flags(), entry="tm16", ldx=2 * C, xchunk=C // 4)
    assert torch.equal(view16, got)


def test_bias_major_map_equals_the_problem_major_map():
    """The 8-problem case takes the bias-major workgroup map (rp_major == 1 needs B G >= 8: the rule covers both 16-bit formats); the
    same problems four at a time take the problem-major one (knn_map, csrc/gkg_knn_common.h)."""
    shape = R.FORMS[3]
    B, G, c, N, M, k, d = _dims(shape)
    assert B == 8 and G == 1
    case, got = A._case(shape), _graph(shape)
    for lo in (0, 4):
        part = call((4, G, c, N, M, k, d), case["x_tm"][lo:lo + 4].contiguous(), case["y_tm"][lo:lo + 4].contiguous(), case["rp_dev"], _flags())
        assert torch.equal(part, got[lo:lo + 4]), f"problems {lo}..{lo + 3}"


@pytest.mark.parametrize("dtype", ("BF16", "F16"))
@pytest.mark.parametrize("shape", [R.FORMS[i] for i in (0, 2, 4)], ids=R.shape_id)
def test_half_precision_features_equal_their_widened_values(shape, dtype):
    case, dims = A._case(shape), _dims(shape)
    td = torch.bfloat16 if dtype == "BF16" else torch.float16
    xh = case["x_tm"].to(td)
    yh = None if case["y_tm"] is None else case["y_tm"].to(td)
    want = call(dims, xh.float(), None if yh is None else yh.float(), case["rp_dev"], _flags())
    got = call(dims, xh, yh, case["rp_dev"], _flags(), dtype=dtype)
    assert torch.equal(got, want)
    B = dims[0]
    cm = lambda t: None if t is None else t.transpose(1, 2).reshape(B * dims[1], dims[2], -1).contiguous()      # noqa: E731
    got_cm = call(dims, cm(xh), cm(yh), case["rp_dev"], _flags(), entry="cm", dtype=dtype)
    assert torch.equal(got_cm, want), "channel-major"


# ------------------------------------------------------------------------------------------------------------------ (c) exact ties
@pytest.mark.parametrize("bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("shape", A.TIE_SHAPES, ids=("one-split", "two-splits", "solo"))
def test_exact_ties_go_to_the_smaller_index(shape, bias):
    """A.test_exact_ties_go_to_the_smaller_index with the fp16 flag: keys (and bias columns) m, m + T, m + 2 T identical for
    m < T = M // 3, so 'smaller index first' alone decides; k d = 8 and 16 end the list inside a group of tied keys."""
    B, G, c, N, M_ = shape
    M = N if M_ is None else M_
    T, k = M // 3, 8
    rng = np.random.default_rng([B, G, c, N, M, int(bias)])
    x = rng.standard_normal((B * G, c, N)).astype(np.float32)
    y = x if M_ is None else rng.standard_normal((B * G, c, M)).astype(np.float32)
    rp = -rng.random((N, M)).astype(np.float32) if bias else None
    for j in (1, 2):
        y[:, :, j * T:(j + 1) * T] = y[:, :, :T]
        if bias:
            rp[:, j * T:(j + 1) * T] = rp[:, :T]
    y_tm = None if M_ is None else _dev(R.to_tm(y, B))
    x_tm, rp_dev = _dev(R.to_tm(x, B)), _dev(rp)
    for d in (1, 2):
        graphs = [call((B, G, c, N, M, k, d), x_tm, y_tm, rp_dev, _flags(s)) for s in SELECT]
        for s, g in zip(SELECT[1:], graphs[1:]):
            assert torch.equal(g, graphs[0]), f"d={d}: the {s} selection differs from the rule's"
        got = graphs[0]
        assert int(got.min()) >= 0 and int(got.max()) < M
        valid = got < 3 * T
        copy, cls = got // T, got % T
        assert int((valid & (copy > 0)).sum()) > got.numel() // 8, "the case does not exercise ties"
        before = A._earlier_same(cls, valid)
        kk = got.shape[-1]
        same = (cls[..., :, None] == cls[..., None, :]) & valid[..., :, None] & valid[..., None, :]
        later = torch.ones(kk, kk, dtype=torch.bool, device="cuda").triu(1)              # [j, i]: i > j
        wrong = same & later & (got[..., None, :] < got[..., :, None])
        assert not bool(wrong.any()), f"d={d}: {int(wrong.sum())} pairs of tied keys in descending index order, first {torch.nonzero(wrong)[0].tolist()}"
        if d == 1:
            missing = valid & (before != copy)
            assert not bool(missing.any()), (f"d=1: {int(missing.sum())} returned copies whose smaller copies are not all at earlier ranks, first "
                                             f"{torch.nonzero(missing)[0].tolist()}")


# ------------------------------------------------------------------------------------------------------------------ (d) the flush
FLUSH_DIMS = (2, 1, 16, 70, 160, 8, 1)            # B, G, c, N, M = 2 T, k, d; no bias
SUB_CH = 5                                        # the channel that carries the subnormal


def _flush_case():
    """Queries: standard normal (norm about 4) with channel SUB_CH = +-1.2e-4, i.e. about 3e-5 normalised — an fp16 subnormal.  Keys:
    0.22 x standard normal with channel SUB_CH = +-0.5 (norm about 1, so about 0.5 normalised); key m + T is key m with that
    channel's sign flipped: the same norm chain and the same |th|^2 chain (they see the channel's square), and distances that differ
    only through the query's channel SUB_CH."""
    B, G, c, N, M, k, d = FLUSH_DIMS
    T = M // 2
    rng = np.random.default_rng(16)
    x = rng.standard_normal((B * G, c, N)).astype(np.float32)
    x[:, SUB_CH, :] = 1.2e-4 * rng.choice([-1.0, 1.0], (B * G, N)).astype(np.float32)
    y = (0.22 * rng.standard_normal((B * G, c, M))).astype(np.float32)
    y[:, SUB_CH, :T] = 0.5 * rng.choice([-1.0, 1.0], (B * G, T)).astype(np.float32)
    y[:, :, T:] = y[:, :, :T]
    y[:, SUB_CH, T:] = -y[:, SUB_CH, :T]
    return x, y, T


def test_the_flush_is_the_definitions():
    """Under the definition the query's channel is 0 and the pair (m, m + T) ties exactly, so the two must appear in ascending index
    order wherever a row lists both; a kernel that kept the subnormal would separate them by about 4 x 3e-5 x 0.5 = 6e-5 >> 2 E =
    6.6e-6 and order them by the sign of that channel — descending for about half of them."""
    from oracle import c_oracle as O
    B, G, c, N, M, k, d = FLUSH_DIMS
    x, y, T = _flush_case()
    xh, _ = O.token_prep(x, True)
    yh, sqy = O.token_prep(y, True)
    sub = np.abs(xh[:, SUB_CH, :])
    assert sub.min() > 1e-5 and sub.max() < 2.0 ** -14, "the query channel is an fp16 subnormal after normalisation"
    assert np.array_equal(sqy[:, :T], sqy[:, T:]) and np.array_equal(np.abs(yh[:, :, :T]), np.abs(yh[:, :, T:])), "the pairs share norm and |th|^2"
    assert 0.3 < np.abs(yh[:, SUB_CH, :]).min() and 4 * sub.min() * np.abs(yh[:, SUB_CH, :]).min() > 3 * 2 * H.bound(c, None)
    x_tm, y_tm = _dev(R.to_tm(x, B)), _dev(R.to_tm(y, B))
    graphs = [call(FLUSH_DIMS, x_tm, y_tm, None, _flags(s)) for s in SELECT]
    for s, g in zip(SELECT[1:], graphs[1:]):
        assert torch.equal(g, graphs[0]), s
    got = graphs[0]
    D, topd, topi = judged(got, x, y, None, c, k, d, "flush")
    assert torch.equal(D[:, :, :T], D[:, :, T:]), "the definition ties every pair exactly"
    cls, hi = got % T, got >= T
    same = cls[..., :, None] == cls[..., None, :]                                         # [j, i]
    later = torch.ones(k, k, dtype=torch.bool, device="cuda").triu(1)                     # i > j
    both = same & later
    assert int(both.any(-1).any(-1).sum()) > got.shape[0] * got.shape[1] // 8, "the case does not exercise the pairs"
    wrong = both & hi[..., :, None] & ~hi[..., None, :]                                   # the larger index at the earlier rank
    assert not bool(wrong.any()), f"{int(wrong.sum())} tied pairs in descending index order (the subnormal reached the distance), first {torch.nonzero(wrong)[0].tolist()}"


def test_subnormal_key_channels_are_zeros():
    """The key side: keys whose channel SUB_CH is about 2e-5 after normalisation give the graph of the same keys with that channel
    exactly 0 — the tiny square changes neither chain (checked on the host), so under the definition the two problems are one."""
    from oracle import c_oracle as O
    B, G, c, N, M, k, d = FLUSH_DIMS
    rng = np.random.default_rng(17)
    x = (0.22 * rng.standard_normal((B * G, c, N))).astype(np.float32)
    x[:, SUB_CH, :] = 0.5 * rng.choice([-1.0, 1.0], (B * G, N)).astype(np.float32)
    y0 = rng.standard_normal((B * G, c, M)).astype(np.float32)
    y0[:, SUB_CH, :] = 0.0
    y1 = y0.copy()
    y1[:, SUB_CH, :] = 8e-5 * rng.choice([-1.0, 1.0], (B * G, M)).astype(np.float32)
    (h0, s0), (h1, s1) = O.token_prep(y0, True), O.token_prep(y1, True)
    keep = np.arange(c) != SUB_CH
    assert np.array_equal(h0[:, keep], h1[:, keep]) and np.array_equal(s0, s1) and np.abs(h1[:, SUB_CH]).max() < 2.0 ** -14
    x_tm = _dev(R.to_tm(x, B))
    g0 = call(FLUSH_DIMS, x_tm, _dev(R.to_tm(y0, B)), None, _flags())
    g1 = call(FLUSH_DIMS, x_tm, _dev(R.to_tm(y1, B)), None, _flags())
    assert torch.equal(g0, g1), f"{int((g0 != g1).sum())} positions differ: a subnormal key channel reached the distance"


# ------------------------------------------------------------------------------------------------------------------ (e) edge inputs
@pytest.mark.parametrize("shape", [(1, 2, 24, 70, 150, 9, 1, False), (2, 2, 40, 80, 1000, 9, 1, False)], ids=R.shape_id)
def test_zero_norm_tokens(shape):
    """All-zero keys have th = 0 and |th|^2 = 0: distance exactly 0 to every query, ties among them broken by index.  An all-zero
    query sees dist = |yh|^2 exactly: its row is the reference's, zero keys first."""
    B, G, c, N, M, k, d, _ = shape
    case = R.make_case(shape, seed=2)
    zk = [3, 40, 41, M - 1]
    case["y"][:, :, zk] = 0.0
    case["x"][0, :, 5] = 0.0
    x, y = _dev(R.to_tm(case["x"], B)), _dev(R.to_tm(case["y"], B))
    graphs = [call(_dims(shape), x, y, None, _flags(s)) for s in SELECT]
    for s, g in zip(SELECT[1:], graphs[1:]):
        assert torch.equal(g, graphs[0]), s
    got = graphs[0]
    D, topd, topi = judged(got, case["x"], case["y"], None, c, k, d, "zero-norm " + R.shape_id(shape))
    assert torch.equal(got[0, 5], topi[0, 5, :k]) and got[0, 5, :4].tolist() == zk
    assert bool((D[:, :, zk] == 0).all())
    isz = torch.zeros(M, dtype=torch.bool, device="cuda")
    isz[zk] = True
    z = isz[got]
    ordinal = torch.cumsum(isz.long(), 0)[got] - 1
    assert int(z.sum()) > 4 * got.shape[0] * got.shape[1] // 10, "the case does not exercise the zero keys"
    before = (torch.cumsum(z.long(), -1) - z.long())
    assert bool((before[z] == ordinal[z]).all()), "zero keys out of index order"


@pytest.mark.parametrize("shape", [(1, 2, 24, 70, 150, 9, 1, True), (2, 2, 40, 80, 1000, 9, 1, False)], ids=R.shape_id)
def test_non_finite_inputs_stay_in_range_and_poison_only_their_own_distances(shape):
    """One NaN token and one Inf feature (its token normalises to 0 ... NaN ... 0) among the queries and among the keys.  Every index
    stays in [0, M), the guards stay intact; a non-finite key's distances are NaN, which no list takes, so the rows of the finite
    queries are judged against the reference over the finite keys."""
    B, G, c, N, M, k, d, bias = shape
    BG = B * G
    case = R.make_case(shape, seed=3)
    case["x"][0, :, 3] = np.nan
    case["x"][BG - 1, 2, 7] = np.inf
    case["y"][0, :, 5] = np.nan
    case["y"][BG - 1, 1, 9] = np.inf
    rows = torch.ones(BG, N, dtype=torch.bool)
    rows[0, 3] = rows[BG - 1, 7] = False
    x, y, rp = _dev(R.to_tm(case["x"], B)), _dev(R.to_tm(case["y"], B)), _dev(case["rp"])
    for s in SELECT:
        got = call(_dims(shape), x, y, rp, _flags(s))
        assert int(got.min()) >= 0 and int(got.max()) < M, s
        D, _, _ = judged(got, case["x"], case["y"], case["rp"], c, k, d, f"non-finite {s} " + R.shape_id(shape), rows=rows.cuda())
        assert bool(torch.isinf(D[0, :, 5]).all()) and bool(torch.isinf(D[BG - 1, :, 9]).all()) and bool(torch.isinf(D[0, 3]).all())
        assert not bool((got[0][rows[0].cuda()] == 5).any()) and not bool((got[BG - 1][rows[BG - 1].cuda()] == 9).any()), s + ": a NaN key was returned"


# ------------------------------------------------------------------------------------------------------------------ (f) rejections
def test_rejected_calls_return_the_documented_code_and_write_nothing():
    lib = A._L().load()
    B, G, c, N, M, k, d = 2, 2, 16, 70, 90, 9, 1
    C, BG = G * c, B * G
    x = torch.randn(B, N, C, device="cuda")
    y = torch.randn(B, M, C, device="cuda")
    hf = _flags()
    UNS = _K("ERR_UNSUPPORTED")
    nbytes = int(lib.gkg_knn_workspace_bytes(BG, c, N, M, k, d, _K("F32"), hf))
    assert nbytes == int(lib.gkg_knn_workspace_bytes(BG, c, N, M, k, d, _K("F32"), _flags(f16=False, bf16=True))) > 0

    def outputs():
        return Buf((nbytes,), torch.uint8), Buf((BG, N, k), torch.int64, fill=A.FILL), Buf((BG, N, k), torch.int64, fill=A.FILL)

    def untouched(what, *bufs):
        torch.cuda.synchronize()
        for b in bufs:
            if isinstance(b.fill, float):
                assert bool(torch.isnan(b.full).all()), what + ": output written"
            else:
                assert bool((b.full == b.fill).all()), what + ": output written"

    # the three k-NN entries, per bad flag word
    bad = {"without GKG_KNN_NORMALIZE": _flags(normalize=False), "with GKG_KNN_BF16_CONTRACT": _flags(bf16=True),
           "with GKG_KNN_X_PREPARED": hf | _K("KNN_X_PREPARED"), "with GKG_KNN_Y_PREPARED": hf | _K("KNN_Y_PREPARED"),
           "with both _PREPARED": hf | _K("KNN_X_PREPARED") | _K("KNN_Y_PREPARED")}
    xcm = x.transpose(1, 2).reshape(BG, c, N).contiguous()
    ycm = y.transpose(1, 2).reshape(BG, c, M).contiguous()
    for what, f in bad.items():
        ws, idx, ctr = outputs()
        rc = lib.gkg_knn_fwd_tm(_p(x), 0, 0, _p(y), None, _p(idx.t), _p(ctr.t), B, G, c, N, M, k, d, _K("F32"), f, _p(ws.t), nbytes, _st())
        assert rc == UNS, f"gkg_knn_fwd_tm {what}: returned {rc}"
        rc = lib.gkg_knn_fwd(_p(xcm), _p(ycm), None, _p(idx.t), _p(ctr.t), BG, c, N, M, k, d, _K("F32"), f, _p(ws.t), nbytes, _st())
        assert rc == UNS, f"gkg_knn_fwd {what}: returned {rc}"
        i16 = Buf((BG, N, k), torch.int16, fill=A.FILL)
        rc = lib.gkg_knn_fwd_tm16(_p(x), 0, 0, _p(y), None, _p(i16.t), B, G, c, N, M, k, d, _K("F32"), f, _p(ws.t), nbytes, _st())
        assert rc == UNS, f"gkg_knn_fwd_tm16 {what}: returned {rc}"
        untouched(what, ws, idx, ctr, i16)

    # as knn_flags of the preparing producers
    ac = torch.ones(C, device="cuda")
    ws, idx, ctr = outputs()
    out = Buf((B * N, C), torch.float32)
    rc = lib.gkg_affine_knn_prep(_p(x), _p(ac), _p(ac), _p(out.t), 0, 0, B, G, c, N, M, k, d, 1, 0, hf, 0, 0, None, None, _p(ws.t), nbytes, _st())
    assert rc == UNS, f"flag as knn_flags of gkg_affine_knn_prep: returned {rc}"
    untouched("gkg_affine_knn_prep", ws, out)

    sums = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    stats = [Buf((C,), torch.float32) for _ in range(4)]                  # a, c_out, mean, invstd
    common = (_p(x), _p(sums), _p(ac), _p(ac), None, None, None, None, *(_p(s.t) for s in stats), _p(out.t), 0, 0, B, G, c, N, M, k, d, 1, 0,
              hf, 0, 0, None, None, _p(ws.t), nbytes, 0.1, 1e-5, None, 0)
    rc = lib.gkg_bn_apply_knn_prep(*common, _st())
    assert rc == UNS, f"flag as knn_flags of gkg_bn_apply_knn_prep: returned {rc}"
    count = torch.full((1,), float(B * N), dtype=torch.float64, device="cuda")
    rc = lib.gkg_bn_apply_knn_prep_sync(*common, _p(count), None, _st())
    assert rc == UNS, f"flag as knn_flags of gkg_bn_apply_knn_prep_sync: returned {rc}"
    untouched("gkg_bn_apply_knn_prep[_sync]", ws, out, *stats)

    xb = torch.randn(B * N, 32, device="cuda").bfloat16()
    wpl = torch.zeros(32 * C, dtype=torch.bfloat16, device="cuda")          # never read: the scope check comes first
    scratch = Buf((64,), torch.uint8)
    assert lib.gkg_linear_bf16_knn_prep_supported(32, B, G, c, N, M, k, d, 1, 0, _flags(f16=False), 0) == 1
    assert lib.gkg_linear_bf16_knn_prep_supported(32, B, G, c, N, M, k, d, 1, 0, hf, 0) == 0
    rc = lib.gkg_linear_bf16_knn_prep(_p(xb), 32, _p(wpl), 32, _p(ac), _p(ac), _p(out.t), 0, 0, B, G, c, N, M, k, d, 1, 0, hf, 0, 0, None, None,
                                      _p(ws.t), nbytes, _p(scratch.t), 64, _st())
    assert rc == UNS, f"flag as knn_flags of gkg_linear_bf16_knn_prep: returned {rc}"
    untouched("gkg_linear_bf16_knn_prep", ws, out, scratch)

    # the fused k-NN + aggregation
    assert lib.gkg_knn_mr_fused_supported(B, G, c, N, M, k, d, 1, 0, _flags(f16=False)) == 1
    assert lib.gkg_knn_mr_fused_supported(B, G, c, N, M, k, d, 1, 0, hf) == 0
    xm, arg = Buf((B * N, 2 * C), torch.float32), Buf((B, N, C), torch.int16, fill=A.FILL)
    rc = lib.gkg_knn_mr_fwd_tm(_p(x), C, 0, _p(y), None, _p(xm.t), _p(arg.t), None, _p(idx.t), _p(ctr.t), B, G, c, N, M, k, d, hf,
                               _p(ws.t), nbytes, _st())
    assert rc == UNS, f"gkg_knn_mr_fwd_tm with the flag: returned {rc}"
    untouched("gkg_knn_mr_fwd_tm", ws, idx, ctr, xm, arg)

    # the size checks of the other forms hold here too
    rc = lib.gkg_knn_fwd_tm(_p(x), 0, 0, _p(y), None, _p(idx.t), _p(ctr.t), B, G, c, N, M, k, d, _K("F32"), hf, _p(ws.t), nbytes - 1, _st())
    assert rc == _K("ERR_WORKSPACE"), f"workspace one byte short: returned {rc}"
    rc = lib.gkg_knn_fwd_tm(_p(x), 0, 0, _p(y), None, _p(idx.t), _p(ctr.t), B, G, c, N, M, 46, 2, _K("F32"), hf, _p(ws.t), nbytes, _st())
    assert rc == _K("ERR_SHAPE"), f"k d > M: returned {rc}"
    untouched("workspace one byte short / k d > M", ws, idx, ctr)


def test_narrow_groups_ignore_the_flag():
    """c = 8 (cpad < 16): the flag is ignored and the call is the bit-exact fp32 contract — the C oracle's graph."""
    from oracle import c_oracle as O
    shape = (2, 2, 8, 100, 130, 5, 2, True)
    case, dims = R.make_case(shape), _dims(shape)
    want, _ = O.knn(case["x"], case["y"], case["rp"], 5, 2)
    x, y, rp = _dev(R.to_tm(case["x"], 2)), _dev(R.to_tm(case["y"], 2)), _dev(case["rp"])
    for select in SELECT:
        on = call(dims, x, y, rp, _flags(select))
        off = call(dims, x, y, rp, _flags(select, f16=False))
        assert torch.equal(on, off), select
        assert np.array_equal(on.cpu().numpy(), want), select


# ------------------------------------------------------------------------------------------------------------------ (g) other forms
@pytest.mark.parametrize("shape", [R.FORMS[1], R.FORMS[4]], ids=R.shape_id)
def test_the_other_forms_are_what_they_were(shape):
    """The element format is a template parameter of one kernel source: the no-flag graph is still the C oracle's, bit for bit, and the
    bf16-flag graph still computes the bf16 definition (R.reference + judge, the existing test's check) — against the references,
    never against saved outputs."""
    from oracle import c_oracle as O
    B, G, c, N, M_, k, d, bias = shape
    case, dims = A._case(shape), _dims(shape)
    exact = call(dims, case["x_tm"], case["y_tm"], case["rp_dev"], _flags(f16=False))
    want, _ = O.knn(case["x"], case["y"], case["rp"], k, d)
    assert np.array_equal(exact.cpu().numpy(), want), "the exact form differs from the C oracle"
    A.judged(A._graph(shape), case["x"], case["y"], case["rp"], c, k, d, "bf16 flag " + R.shape_id(shape))
    dbf, dhf = int((A._graph(shape) != exact).sum()), int((_graph(shape) != exact).sum())
    print(f"knn_f16 {R.shape_id(shape)}: positions differing from the exact graph: bf16 {dbf}, fp16 {dhf} of {exact.numel()}")
