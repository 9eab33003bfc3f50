"""The bf16-contraction k-NN (GKG_KNN_BF16_CONTRACT: csrc/gkg_knn_bf.hip, knn_tile_kernel<..., BF = true>) through the C ABI, against
the fp64 evaluation of its definition in tests/knn_bf16_ref.py (definition, bound E and its derivation: that module's docstring).

EVERY CALL.  gkg_knn_fwd / gkg_knn_fwd_tm / gkg_knn_fwd_tm16 straight from the library; the workspace has exactly
gkg_knn_workspace_bytes(...) bytes and sits between guard bands, and so do the index and centre planes.  After the call: guards
intact, center == n.  A graph that is judged: every index in [0, M), the k entries of a row distinct, at every kept rank the
definition distance of the returned key within 2 E of the reference's, and the share of positions that differ from the reference
ranking at most the case's near-tie share (<= 5 %: tests/test_knn_bf16_reference_host.py).  Each case prints its mismatch share and
its largest tolerated gap / 2E under ``pytest -s`` (figures: EXPERIMENTS.md "bf16-contraction k-NN at the C ABI").

FORMS (R.FORMS: B, G, c, N, M or self, k, d, bias), after knn_plan (csrc/gkg_knn_plan.h; held to these claims by tests/test_knn_plan_host.py).
Query tiles are 64 wide, key tiles 32; S = key splits (knn_pick_splits: only below 256 workgroups, at least 8 key tiles per split), tps =
key tiles per split; the list size KD is the first of 9, 18, 27, 36, 64 that holds k d; cp16 = c rounded up to 16.  The rule takes the
buffered selection when tps >= 8 and (tps >= 16 or KD >= 18 or S > 1); the candidate buffer has 16 entries per lane if the query image
64 (cp16 + 8) 2 B plus 33 KB fits the workgroup's LDS share (160 KB / 3 with a bias and KD <= 18, / 2 with a bias otherwise; without
a bias / 4, / 3, / 2 for KD <= 12, <= 27, above), else 12 if it fits with 25 KB, else none; 9-entry lists always use 12.
    (2, 1, 12, 77, self, 3, 2, bias)      c 12 -> cp16 16; two query tiles, the second ragged; 3 key tiles, S = 1: direct by rule; KD 9
    (2, 4, 80, 324, self, 9, 1, bias)     cfg2-like; 48 workgroups, 11 key tiles: S = 2 with a bias -> partial lists + knn_merge_kernel
    (2, 2, 40, 80, 1000, 9, 1, none)      few queries, many keys: S = 4 (tps 8), the no-bias instantiation, buffered by rule, last key tile of 8
    (8, 1, 40, 4100, 300, 9, 2, bias)     65 query tiles x 8 problems with a bias and cp16 = 48 <= 64: bias-major map (rp_major == 1) on a grid
                                          padded to 72 x 8, last query tile of 4; 520 workgroups < 2048: four waves; KD 18, 16-entry buffers
    (32, 1, 12, 4100, 520, 9, 1, bias)    2080 workgroups, query image 3 KB: single-wave workgroups (solo) AND the bias-major map; 12 entries
    (32, 1, 12, 4100, 520, 18, 1, none)   solo, KD 18 (16-entry buffers, merge network), no bias, problem-major map
    (1, 2, 200, 300, self, 9, 2, bias)    cp16 208: the 27 KB query image leaves room for 12-entry buffers only (KD 18); S = 2
    (1, 1, 320, 200, self, 9, 3, bias)    KD 27; widest group.  Direct by rule because the stream is short (tps = 7); its 41 KB query image
                                          still fits 16-entry buffers in the 80 KB share of a KD 27 workgroup, which the forced form takes
    (1, 1, 320, 200, self, 9, 2, bias)    the same image against the 53 KB share of a KD 18 workgroup: no room for any buffer, direct by rule;
                                          GKG_KNN_SELECT_BUFFERED forces 12 entries -> 66 KB of LDS, above the 64 KB default limit
    (2, 1, 48, 300, self, 18, 2, bias)    KD 36; S = 2
    (1, 1, 16, 100, 333, 32, 2, none)     KD 64: direct only, whatever the flag; M % 4 != 0; S = 2
    (1, 1, 33, 65, 130, 5, 1, bias)       odd c, cp16 = 48; a second query tile of one row; M % 4 == 2 with a bias
Each with flags auto, GKG_KNN_SELECT_DIRECT and GKG_KNN_SELECT_BUFFERED: the three graphs are identical bit for bit (the selection
never touches the arithmetic) — which also compares the solo form with the four-wave direct form on the same inputs."""
import functools

import numpy as np
import pytest
import torch

import knn_bf16_ref as R
from util import Buf, xm_pack

pytestmark = pytest.mark.gpu

FILL = -7                                  # what the index / centre planes hold before a call
SELECT = ("auto", "direct", "buffered")


def _L():
    from gkgnet_amd import _lib
    return _lib


def _K(name):
    return _L()._K[name]


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    from gkgnet_amd.ops import _stream
    return _stream()


def _flags(select="auto", normalize=True, bf16=True):
    f = (_K("KNN_NORMALIZE") if normalize else 0) | (_K("KNN_BF16_CONTRACT") if bf16 else 0)
    return f | {"auto": 0, "direct": _K("KNN_SELECT_DIRECT"), "buffered": _K("KNN_SELECT_BUFFERED")}[select]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def call(dims, x, y, rp, flags, entry="tm", dtype="F32", ldx=0, xchunk=0, center=True, what=""):
    """One k-NN call between guard bands.  dims (B, G, c, N, M, k, d); x / y device tensors in the entry's layout (token-major (B, T, C)
    for 'tm' / 'tm16', channel-major (B G, c, T) for 'cm'), rp (N, M) or None.  -> the neighbour lists (B G, N, k) int64, on the device."""
    lib = _L().load()
    B, G, c, N, M, k, d = dims
    BG = B * G
    what = what or f"{entry} {dims} flags={flags}"
    nbytes = int(lib.gkg_knn_workspace_bytes(BG, c, N, M, k, d, _K(dtype), flags))
    assert nbytes > 0, what
    ws = Buf((nbytes,), torch.uint8)
    u16 = entry == "tm16"
    idx = Buf((BG, N, k), torch.int16 if u16 else torch.int64, fill=FILL)
    ctr = Buf((BG, N, k), torch.int64, fill=FILL) if center and not u16 else None
    if entry == "cm":
        rc = lib.gkg_knn_fwd(_p(x), _p(y), _p(rp), _p(idx.t), _p(ctr.t) if ctr else None, BG, c, N, M, k, d, _K(dtype), flags,
                             _p(ws.t), nbytes, _st())
    elif u16:
        rc = lib.gkg_knn_fwd_tm16(_p(x), ldx, xchunk, _p(y), _p(rp), _p(idx.t), B, G, c, N, M, k, d, _K(dtype), flags, _p(ws.t), nbytes, _st())
    else:
        rc = lib.gkg_knn_fwd_tm(_p(x), ldx, xchunk, _p(y), _p(rp), _p(idx.t), _p(ctr.t) if ctr else None, B, G, c, N, M, k, d, _K(dtype),
                                flags, _p(ws.t), nbytes, _st())
    _L().check(rc, what)
    torch.cuda.synchronize()
    assert ws.guards_ok(), what + ": wrote outside its workspace"
    assert idx.guards_ok(), what + ": wrote outside the index plane"
    if ctr is not None:
        assert ctr.guards_ok(), what + ": wrote outside the centre plane"
        assert torch.equal(ctr.t, torch.arange(N, device="cuda").view(1, N, 1).expand(BG, N, k)), what + ": center != n"
    return (idx.t.long() & 0xFFFF) if u16 else idx.t.clone()


def _dims(shape):
    B, G, c, N, M_, k, d, _ = shape
    return (B, G, c, N, N if M_ is None else M_, k, d)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The shared inputs of a FORMS shape: the numpy case of R.make_case plus its device tensors; never modified."""
    case = R.make_case(shape)
    B = shape[0]
    case.update(x_tm=_dev(R.to_tm(case["x"], B)), y_tm=None if case["y"] is None else _dev(R.to_tm(case["y"], B)), rp_dev=_dev(case["rp"]))
    return case


@functools.lru_cache(maxsize=None)
def _graph(shape):
    """The graph of a FORMS shape by the library's own rule (token-major entry, int64 lists): what every invariance compares with."""
    case = _case(shape)
    return call(_dims(shape), case["x_tm"], case["y_tm"], case["rp_dev"], _flags("auto"))


def judged(got, x, y, rp, c, k, d, what, normalize=True, rows=None):
    """Reference, bound and judge for one graph; asserts the mismatch share against the near-tie share of the judged rows and prints
    the case's figures.  x, y, rp: numpy, channel-major.  -> (D, topd, topi) for further assertions."""
    D, topd, topi = R.reference(x, y, rp, k, d, normalize=normalize, device="cuda")
    E = R.bound(c, rp, R.scale(x, y, normalize))
    near = R.near_tie_share(topd if rows is None else topd[rows.to(topd.device)], E, k, d)
    share, worst = R.judge(got, D, topd, topi, k, d, E, rows=rows, what=what)
    print(f"knn_bf16 {what}: mismatch {100 * share:.4f} % (near ties {100 * near:.3f} %), worst gap/2E {worst:.3f}")
    assert share <= near, f"{what}: mismatch share {share:.5f} above the near-tie share {near:.5f}"
    return D, topd, topi


# ------------------------------------------------------------------------------------------------------------------ (a) forms
@pytest.mark.parametrize("shape", R.FORMS, ids=R.shape_id)
def test_every_form_computes_the_definition(shape):
    B, G, c, N, M_, k, d, bias = shape
    case = _case(shape)
    got = _graph(shape)
    _, topd, _ = judged(got, case["x"], case["y"], case["rp"], c, k, d, R.shape_id(shape))
    assert R.near_tie_share(topd, R.bound(c, case["rp"]), k, d) <= R.NEAR_TIE_CAP
    for select in ("direct", "buffered"):
        other = call(_dims(shape), case["x_tm"], case["y_tm"], case["rp_dev"], _flags(select))
        assert torch.equal(other, got), f"{R.shape_id(shape)}: the {select} selection differs from the rule's at {int((other != got).sum())} positions"


# ------------------------------------------------------------------------------------------------------------------ (b) invariances
@pytest.mark.parametrize("shape", R.FORMS, ids=R.shape_id)
def test_entry_points_and_list_formats_agree(shape):
    """Channel-major gkg_knn_fwd, the u16 lists of gkg_knn_fwd_tm16 and a call without a centre plane give the token-major graph."""
    case, got, dims = _case(shape), _graph(shape), _dims(shape)
    cm = call(dims, _dev(case["x"]), _dev(case["y"]), case["rp_dev"], _flags(), entry="cm")
    assert torch.equal(cm, got), "channel-major entry"
    u16 = call(dims, case["x_tm"], case["y_tm"], case["rp_dev"], _flags(), entry="tm16")
    assert torch.equal(u16, got), "u16 lists"
    bare = call(dims, case["x_tm"], case["y_tm"], case["rp_dev"], _flags(), center=False)
    assert torch.equal(bare, got), "center == NULL"


def test_bias_major_map_equals_the_problem_major_map():
    """The 8-problem case takes the bias-major workgroup map (rp_major == 1 needs B G >= 8); the same problems four at a time take
    the problem-major one (knn_map, csrc/gkg_knn_common.h)."""
    shape = R.FORMS[3]
    B, G, c, N, M, k, d = _dims(shape)
    assert B == 8 and G == 1
    case, got = _case(shape), _graph(shape)
    for lo in (0, 4):
        part = call((4, G, c, N, M, k, d), case["x_tm"][lo:lo + 4].contiguous(), case["y_tm"][lo:lo + 4].contiguous(), case["rp_dev"], _flags())
        assert torch.equal(part, got[lo:lo + 4]), f"problems {lo}..{lo + 3}"


@pytest.mark.parametrize("dtype", ("BF16", "F16"))
@pytest.mark.parametrize("shape", [R.FORMS[i] for i in (0, 2, 4)], ids=R.shape_id)
def test_half_precision_features_equal_their_widened_values(shape, dtype):
    case, dims = _case(shape), _dims(shape)
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


@pytest.mark.parametrize("shape", [R.FORMS[i] for i in (1, 6, 9, 10)], ids=R.shape_id)
def test_x_as_the_x_half_of_an_xm_buffer(shape):
    """x passed as a view (ldx = 2 C, xchunk = C / 4: include/gkg_hip.h "XM layout"); the m half holds NaN."""
    case, got, dims = _case(shape), _graph(shape), _dims(shape)
    B, G, c, N = dims[:4]
    C = G * c
    assert C % 16 == 0 and c % 4 == 0
    x2 = case["x_tm"].reshape(B * N, C)
    XM = xm_pack(x2, torch.full_like(x2, float("nan"))).contiguous()
    view = call(dims, XM, case["y_tm"], case["rp_dev"], _flags(), ldx=2 * C, xchunk=C // 4)
    assert torch.equal(view, got)
    view16 = call(dims, XM, case["y_tm"], case["rp_dev"], _flags(), entry="tm16", ldx=2 * C, xchunk=C // 4)
    assert torch.equal(view16, got)


def test_narrow_groups_ignore_the_flag():
    """c = 8 (cpad < 16): the flag is ignored and the call is the bit-exact fp32 contract — the C oracle's graph."""
    from oracle import c_oracle as O
    shape = (2, 2, 8, 100, 130, 5, 2, True)
    case, dims = R.make_case(shape), _dims(shape)
    want, _ = O.knn(case["x"], case["y"], case["rp"], 5, 2)
    x, y, rp = _dev(R.to_tm(case["x"], 2)), _dev(R.to_tm(case["y"], 2)), _dev(case["rp"])
    for select in SELECT:
        on = call(dims, x, y, rp, _flags(select))
        off = call(dims, x, y, rp, _flags(select, bf16=False))
        assert torch.equal(on, off), select
        assert np.array_equal(on.cpu().numpy(), want), select


def test_without_normalisation():
    """No GKG_KNN_NORMALIZE: th = t; the bound uses the case's own 2 max|bf x| max|bf y| + max |y|^2."""
    shape = (2, 2, 24, 70, 150, 9, 1, True)
    case, dims = R.make_case(shape, seed=1), _dims(shape)
    x, y, rp = _dev(R.to_tm(case["x"], 2)), _dev(R.to_tm(case["y"], 2)), _dev(case["rp"])
    got = call(dims, x, y, rp, _flags(normalize=False))
    judged(got, case["x"], case["y"], case["rp"], 24, 9, 1, "not normalised " + R.shape_id(shape), normalize=False)
    for select in ("direct", "buffered"):
        assert torch.equal(call(dims, x, y, rp, _flags(select, normalize=False)), got), select


# ------------------------------------------------------------------------------------------------------------------ (c) exact ties
def _earlier_same(cls, valid):
    """cls (.., k) integer classes, valid (.., k) bool -> per position the number of EARLIER valid positions of the same class."""
    k = cls.shape[-1]
    same = (cls[..., :, None] == cls[..., None, :]) & valid[..., :, None] & valid[..., None, :]
    earlier = torch.ones(k, k, dtype=torch.bool, device=cls.device).tril(-1)             # [j, i]: i < j
    return (same & earlier).sum(-1)


TIE_SHAPES = [(32, 1, 12, 520, None), (2, 4, 80, 324, None), (32, 1, 12, 4100, 520)]


@pytest.mark.parametrize("bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("shape", TIE_SHAPES, ids=("one-split", "two-splits", "solo"))
def test_exact_ties_go_to_the_smaller_index(shape, bias):
    """Keys (and bias columns) m, m + T, m + 2 T identical for m < T = M // 3: their distances to any query are equal in any
    arithmetic, so 'smaller index first' alone decides.  In a row, the copies of one key must appear in ascending index order; with
    d = 1 (every rank emitted) a returned copy j > 0 must have all its smaller copies at earlier ranks.  k d = 8 and 16 are no
    multiples of 3, so the list ends INSIDE a group of tied keys and the rule also decides who is in it.
    With a bias the key tiles are visited centre-out — a wave meets the larger index of a tied pair first — and the buffered
    threshold must be '<='.  Shapes (B, G, c, N, M or self):
        one-split   288 workgroups: S = 1, four waves, each over 4-5 of the 17 key tiles; buffered by rule (tps 17)
        two-splits  the cfg2-like shape: the copies lie in different key splits (tiles 0-5 | 6-10) and waves
        solo        2080 single-wave workgroups: ONE list per query over all 17 key tiles, so every tie is decided inside it"""
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
        before = _earlier_same(cls, valid)
        # ascending order: every earlier copy of my key has a smaller index, i.e. no LATER position holds a smaller copy
        kk = got.shape[-1]
        same = (cls[..., :, None] == cls[..., None, :]) & valid[..., :, None] & valid[..., None, :]
        later = torch.ones(kk, kk, dtype=torch.bool, device="cuda").triu(1)              # [j, i]: i > j
        wrong = same & later & (got[..., None, :] < got[..., :, None])
        assert not bool(wrong.any()), f"d={d}: {int(wrong.sum())} pairs of tied keys in descending index order, first {torch.nonzero(wrong)[0].tolist()}"
        if d == 1:
            missing = valid & (before != copy)
            assert not bool(missing.any()), (f"d=1: {int(missing.sum())} returned copies whose smaller copies are not all at earlier ranks, first "
                                             f"{torch.nonzero(missing)[0].tolist()}")


# ------------------------------------------------------------------------------------------------------------------ (d) zero-norm tokens
@pytest.mark.parametrize("shape", [(1, 2, 24, 70, 150, 9, 1, False), (2, 2, 40, 80, 1000, 9, 1, False)], ids=R.shape_id)
def test_zero_norm_tokens(shape):
    """All-zero keys have th = 0 and |th|^2 = 0: distance exactly 0 to every query, ties among them broken by index.  An all-zero
    query sees dist = |yh|^2 exactly, in the kernel and in the reference alike: its row is the reference's, zero keys first."""
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
    z = isz[got]                                                                        # (BG, N, k): a zero key at this rank
    ordinal = torch.cumsum(isz.long(), 0)[got] - 1                                      # which of the zero keys
    assert int(z.sum()) > 4 * got.shape[0] * got.shape[1] // 10, "the case does not exercise the zero keys"
    before = (torch.cumsum(z.long(), -1) - z.long())                                    # zero keys at earlier ranks
    assert bool((before[z] == ordinal[z]).all()), "zero keys out of index order"


# ------------------------------------------------------------------------------------------------------------------ (e) non-finite inputs
@pytest.mark.parametrize("shape", [(1, 2, 24, 70, 150, 9, 1, True), (2, 2, 40, 80, 1000, 9, 1, False)], ids=R.shape_id)
def test_non_finite_inputs_stay_in_range_and_poison_only_their_own_distances(shape):
    """One NaN token and one Inf feature (its token normalises to 0 ... NaN ... 0) among the queries and among the keys, at a
    single-split and a split shape.  Every index stays in [0, M), the guards stay intact; a non-finite key's distances are NaN, which
    no list takes, so the rows of the finite queries are judged against the reference over the finite keys."""
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
    lib = _L().load()
    B, G, c, N, M, k, d = 2, 2, 16, 70, 90, 9, 1
    C, BG = G * c, B * G
    x = torch.randn(B, N, C, device="cuda")
    y = torch.randn(B, M, C, device="cuda")
    bf = _flags()
    nbytes = int(lib.gkg_knn_workspace_bytes(BG, c, N, M, k, d, _K("F32"), bf))

    def outputs():
        return Buf((nbytes,), torch.uint8), Buf((BG, N, k), torch.int64, fill=FILL), Buf((BG, N, k), torch.int64, fill=FILL)

    def untouched(what, *bufs):
        torch.cuda.synchronize()
        for b in bufs:
            if isinstance(b.fill, float):
                assert bool(torch.isnan(b.full).all()), what + ": output written"
            else:
                assert bool((b.full == b.fill).all()), what + ": output written"

    ws, idx, ctr = outputs()
    rc = lib.gkg_knn_fwd_tm(_p(x), 0, 0, _p(y), None, _p(idx.t), _p(ctr.t), B, G, c, N, M, k, d, _K("F32"), bf | _K("KNN_X_PREPARED"),
                            _p(ws.t), nbytes, _st())
    assert rc == _K("ERR_UNSUPPORTED"), f"flag with GKG_KNN_X_PREPARED: returned {rc}"
    untouched("flag with GKG_KNN_X_PREPARED", ws, idx, ctr)

    ws, idx, ctr = outputs()
    out = Buf((B * N, C), torch.float32)
    ac = torch.ones(C, device="cuda")
    rc = lib.gkg_affine_knn_prep(_p(x), _p(ac), _p(ac), _p(out.t), 0, 0, B, G, c, N, M, k, d, 1, 0, bf, 0, 0, None, None, _p(ws.t), nbytes, _st())
    assert rc == _K("ERR_UNSUPPORTED"), f"flag as knn_flags of gkg_affine_knn_prep: returned {rc}"
    untouched("flag as knn_flags of gkg_affine_knn_prep", ws, out)

    ws, idx, ctr = outputs()
    rc = lib.gkg_knn_fwd_tm(_p(x), 0, 0, _p(y), None, _p(idx.t), _p(ctr.t), B, G, c, N, M, k, d, _K("F32"), bf, _p(ws.t), nbytes - 1, _st())
    assert rc == _K("ERR_WORKSPACE"), f"workspace one byte short: returned {rc}"
    untouched("workspace one byte short", ws, idx, ctr)

    ws, idx, ctr = outputs()
    rc = lib.gkg_knn_fwd_tm(_p(x), 0, 0, _p(y), None, _p(idx.t), _p(ctr.t), B, G, c, N, M, 46, 2, _K("F32"), bf, _p(ws.t), nbytes, _st())
    assert rc == _K("ERR_SHAPE"), f"k d > M: returned {rc}"
    untouched("k d > M", ws, idx, ctr)
    rc = lib.gkg_knn_fwd(_p(x), _p(y), None, _p(idx.t), _p(ctr.t), BG, c, N, M, 46, 2, _K("F32"), bf, _p(ws.t), nbytes, _st())
    assert rc == _K("ERR_SHAPE"), f"gkg_knn_fwd: k d > M: returned {rc}"
    untouched("gkg_knn_fwd: k d > M", ws, idx, ctr)
