"""csrc/gkg_gconv.hip through the C ABI against the fp64 reference of tests/gconv_ref.py: the four entry points of the GIN sum
(conv='gin') and the graph attention (conv='gat') of include/gkg_hip.h "GIN and graph-attention aggregations".  Operands, p, the
optional outputs and the workspace are the test's own, so nothing of the autograd wrappers enters the comparison.

Shapes (B, C, N, M, k) = gconv_ref.SHAPES, each bipartite (a distinct src buffer) and, where M == N, as a self graph (src NULL):
    (1, 1, 1, 1, 1)                  everything degenerate; GAT k = 1: p == 1, de == 0
    (2, 5, 255 / 256 / 257, 37, 9)   one thread short of a full workgroup, exactly one, a second one with a single live thread
    (2, 6, 37, 257, 5)               M = 257: scan chunks of 2, threads >= 129 empty; the gather grid sized by M > N
    (1, 4, 40, 700, 3)               scan chunks of 3, a ragged last chunk, most keys without an edge
    (3, 8, 513, 513, 3)              self graph, and the same sizes bipartite
    (1, 20, 300, 5, 4)               five keys: sorted lists of ~240 edges each
    (2, 3, 150, 1, 4)                M = 1: one hub of 600 edges per image, all logits of a row equal
    (2, 12, 64, 600, 64)             largest k
    (4, 3, 70, 1000, 6)              M >> N, four images with different graphs
Neighbour lists are randint (repeats), every third row repeats its first neighbour, two entries are out of range (-5, M + 7).

THE BAR (constants, scales and report functions live in gconv_ref so that tests/test_gconv_reference_host.py, which shows on the CPU
that seventeen wrong formulas land above it, cannot drift from this file).  Error = |got - fp64| / scale with the first-order
magnitudes of gconv_ref (*_mag) as scales; yardstick = the same formula in plain torch fp32 on the same operands; the kernel must
satisfy err <= max(4 * yardstick, 2^-22); GIN's geps, an fp64 sum of exact products, 1e-12 of the sum of |term|.  gx on a bipartite
graph, da[:C] and dbias of the attention are 0 in exact arithmetic and are judged against their scales only.  Measured figures per
shape: EXPERIMENTS.md "GIN / GAT kernels vs fp64" (every test prints its own with ``pytest -s``).

Every output sits between guard bands and is pre-filled with NaN; the workspace has exactly gkg_gconv_workspace_bytes bytes between
bands and is full of 0xFF bytes unless a test says otherwise.  Every call asserts the bands untouched."""
import random

import pytest
import torch

import gconv_ref as R
from util import Buf

pytestmark = pytest.mark.gpu

WS_BAND = 256                            # bytes on either side of the workspace (keeps its base 256-byte aligned)


# ------------------------------------------------------------------------------------------------------------------ helpers
def _L():
    from gkgnet_amd import _lib
    return _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    from gkgnet_amd.ops import _stream
    return _stream()


class Ws:
    """A workspace of exactly ``nbytes`` bytes (default: what the shape needs) between two bands of 0xA5, filled with ``fill``."""

    def __init__(self, shape=None, fill=0xFF, nbytes=None):
        self.n = int(_L().load().gkg_gconv_workspace_bytes(*shape)) if nbytes is None else nbytes
        assert self.n > 0
        self.full = torch.full((self.n + 2 * WS_BAND,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t = self.full[WS_BAND:WS_BAND + self.n]
        self.t.fill_(fill)
        assert self.t.data_ptr() % 256 == 0

    def guards_ok(self):
        return bool((self.full[:WS_BAND] == 0xA5).all()) and bool((self.full[-WS_BAND:] == 0xA5).all())


def _dev(k):
    return {n: (v.cuda().contiguous() if torch.is_tensor(v) else v) for n, v in k.items()}


def _done(what, *bufs):
    torch.cuda.synchronize()
    for b in bufs:
        assert b is None or b.guards_ok(), what + " wrote outside its outputs / workspace"


def _gin_fwd(dv):
    B, C, N, M, k = dv["shape"]
    h = Buf((B, C, N))
    _L().check(_L().load().gkg_gin_fwd(_p(dv["x"]), _p(dv["src"]), _p(dv["idx"]), _p(dv["eps"]), _p(h.t), B, C, N, M, k, _st()),
               "gkg_gin_fwd")
    _done("gkg_gin_fwd", h)
    return h.cpu()


def _gin_bwd(dv, ws=None, geps=True, g=None):
    """-> (gx, gsrc or None, geps or None) on the CPU.  ``geps`` False: geps and x are both NULL."""
    B, C, N, M, k = dv["shape"]
    ws = ws or Ws(dv["shape"])
    gx, gs = Buf((B, C, N)), (Buf((B, C, M)) if dv["src"] is not None else None)
    ge = Buf((1,), torch.float64) if geps else None
    _L().check(_L().load().gkg_gin_bwd(_p(dv["g"] if g is None else g), _p(dv["x"]) if geps else None, _p(dv["eps"]), _p(dv["idx"]),
                                       _p(gx.t), None if gs is None else _p(gs.t), None if ge is None else _p(ge.t), B, C, N, M, k,
                                       _p(ws.t), ws.n, _st()), "gkg_gin_bwd")
    _done("gkg_gin_bwd", gx, gs, ge, ws)
    return gx.cpu(), (None if gs is None else gs.cpu()), (None if ge is None else ge.cpu().reshape(()))


def _gat_fwd(dv, ws=None, bias="case"):
    """-> (agg, p) on the CPU and p on the device."""
    B, C, N, M, k = dv["shape"]
    ws = ws or Ws(dv["shape"])
    bias = dv["bias"] if isinstance(bias, str) else bias
    agg, p = Buf((B, C, N)), Buf((B, N, k))
    _L().check(_L().load().gkg_gat_fwd(_p(dv["x"]), _p(dv["src"]), _p(dv["idx"]), _p(dv["a"]), _p(bias), _p(agg.t), _p(p.t), B, C, N, M, k,
                                       _p(ws.t), ws.n, _st()), "gkg_gat_fwd")
    _done("gkg_gat_fwd", agg, p, ws)
    return agg.cpu(), p.cpu(), p.t


def _gat_bwd(dv, p_dev, ws=None, da=True, dbias=True):
    """-> dict(gx, gsrc, da, dbias) on the CPU (None: not requested / self graph)."""
    B, C, N, M, k = dv["shape"]
    ws = ws or Ws(dv["shape"])
    gx, gs = Buf((B, C, N)), (Buf((B, C, M)) if dv["src"] is not None else None)
    dab, dbb = (Buf((2 * C,), torch.float64) if da else None), (Buf((1,), torch.float64) if dbias else None)
    o = lambda b: None if b is None else _p(b.t)                             # noqa: E731
    _L().check(_L().load().gkg_gat_bwd(_p(dv["g"]), _p(dv["x"]), _p(dv["src"]), _p(dv["idx"]), _p(dv["a"]), _p(p_dev), o(gx), o(gs), o(dab),
                                       o(dbb), B, C, N, M, k, _p(ws.t), ws.n, _st()), "gkg_gat_bwd")
    _done("gkg_gat_bwd", gx, gs, dab, dbb, ws)
    c = lambda b: None if b is None else b.cpu()                             # noqa: E731
    return dict(gx=c(gx), gsrc=c(gs), da=c(dab), dbias=None if dbb is None else dbb.cpu().reshape(()))


def _written(*ts):
    return all(t is None or bool(torch.isfinite(t).all()) for t in ts)


def _held(rep, what):
    assert R.passes(rep), (what, rep)


def _same(a, b):
    """The same bits (NaN equal to NaN); None equals None."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


# ------------------------------------------------------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("shape,bip", R.CASES, ids=R.IDS)
def test_gin_against_fp64(shape, bip):
    k = R.make_case(shape, bip)
    dv = _dev(k)
    tag = f"{shape} {'bipartite' if bip else 'self'}"
    h = _gin_fwd(dv)
    assert _written(h)
    _held(R.gin_fwd_report(tag, h, k), "gin_fwd")
    gx, gsrc, geps = _gin_bwd(dv)
    assert _written(gx, gsrc, geps) and (gsrc is not None) == bip
    _held(R.gin_bwd_report(tag, gx, gsrc, geps, k), "gin_bwd")


@pytest.mark.parametrize("shape,bip", R.CASES, ids=R.IDS)
def test_gat_against_fp64(shape, bip):
    """The backward runs twice: with the kernel's own p, and with the fp32 rounding of the fp64 softmax (a p no kernel made: the
    backward is judged independently of the forward).  The reference of each run starts from the p that run was given."""
    B, C, N, M, kk = shape
    k = R.make_case(shape, bip)
    dv = _dev(k)
    tag = f"{shape} {'bipartite' if bip else 'self'}"
    agg, p, p_dev = _gat_fwd(dv)
    assert _written(agg, p)
    _held(R.gat_fwd_report(tag, agg, p, k), "gat_fwd")
    assert bool((p >= 0).all()) and bool((p <= 1).all())
    row = float((p.double().sum(-1) - 1).abs().max())
    print(f"GCONV {tag} gat_fwd: |sum_k p - 1| {row:.3e} (bound {kk * 2.0 ** -23:.3e})")
    assert row <= kk * 2.0 ** -23
    if kk == 1:
        assert bool((p == 1).all())
    got = _gat_bwd(dv, p_dev)
    assert _written(*got.values()) and (got["gsrc"] is not None) == bip
    _held(R.gat_bwd_report(tag + " own p", got, p, k), "gat_bwd, own p")
    p_made = R.gat_fwd(k["x"].double(), None if k["src"] is None else k["src"].double(), k["idx"], k["a"].double(), k["bias"].double())[1].float()
    got = _gat_bwd(dv, p_made.cuda())
    assert _written(*got.values())
    _held(R.gat_bwd_report(tag + " made p", got, p_made, k), "gat_bwd, test-made p")


# ------------------------------------------------------------------------------------------------------------------ exact arithmetic
def _d(t):
    return None if t is None else t.double()


def _bits(got, want, what):
    assert got.dtype in (torch.float32, torch.float64) and torch.equal(got.double(), want), (what, int((got.double() != want).sum()))


@pytest.mark.parametrize("shape,bip", R.CASES, ids=R.IDS)
def test_gin_exact_arithmetic_bit_for_bit(shape, bip):
    """Operands on the 2^-2 grid, eps = 0.25: every product and sum is exact, so order cannot matter.  h, gx, gsrc and geps equal
    fp64 exactly; then gh[b][c][n] = (c + 1) (n + 1), where any dropped, doubled or misplaced edge of the transposed graph changes an
    integer."""
    B, C, N, M, kk = shape
    k = R.make_exact_case(shape, bip)
    dv = _dev(k)
    x, src, idx, eps = _d(k["x"]), _d(k["src"]), k["idx"], _d(k["eps"])
    _bits(_gin_fwd(dv), R.gin_fwd(x, src, idx, eps), "h")
    ramp = ((torch.arange(C).view(1, C, 1) + 1) * (torch.arange(N).view(1, 1, N) + 1)).float().expand(B, C, N).contiguous()
    for name, gh in (("grid", k["g"]), ("ramp", ramp)):
        want = R.gin_bwd(_d(gh), x, eps, idx, M, bip)
        got = _gin_bwd(dv, g=gh.cuda())
        _bits(got[0], want[0], name + " gx")
        if bip:
            _bits(got[1], want[1], name + " gsrc")
        _bits(got[2], want[2], name + " geps")


@pytest.mark.parametrize("shape,bip", R.UNIFORM_SHAPES)
def test_gat_zero_weights_bit_for_bit(shape, bip):
    """a = 0, k a power of two, operands on the 2^-2 grid: p = 1 / k, and agg, gsrc, da[C:] are exact whatever the order; sde is 0,
    so gx of a bipartite graph, da[:C] and dbias are exactly 0."""
    B, C, N, M, kk = shape
    k = R.make_exact_case(shape, bip)
    dv = _dev(k)
    x, src, idx, a, bias, g = _d(k["x"]), _d(k["src"]), k["idx"], _d(k["a"]), _d(k["bias"]), _d(k["g"])
    agg, p, p_dev = _gat_fwd(dv)
    want_agg, want_p = R.gat_fwd(x, src, idx, a, bias)
    assert bool((p == 1.0 / kk).all())
    _bits(p, want_p, "p")
    _bits(agg, want_agg, "agg")
    got, want = _gat_bwd(dv, p_dev), R.gat_bwd(g, x, src, idx, a, want_p)
    for n in ("gx", "da", "dbias") + (("gsrc",) if bip else ()):
        _bits(got[n], want[n], n)
    assert float(got["dbias"]) == 0 and bool((got["da"][:C] == 0).all()) and float(got["da"][C:].abs().max()) > 0


@pytest.mark.parametrize("shape,bip", R.ONE_HOT_SHAPES)
def test_gat_one_hot_bit_for_bit(shape, bip):
    """A key score of 128 x (the key's rank): fp32 expf of every loser is 0, p is exactly one-hot and agg the gather at the list's
    best key (NOT the fp64 softmax, whose losers are e^-128 and more).  The backward on that p is exact on grid operands."""
    k = R.make_one_hot_case(shape, bip)
    dv = _dev(k)
    agg, p, p_dev = _gat_fwd(dv)
    want_p, want_agg = R.one_hot_expect(k)
    assert torch.equal(p, want_p), int((p != want_p).sum())
    assert torch.equal(agg, want_agg), int((agg != want_agg).sum())
    got = _gat_bwd(dv, p_dev)
    want = R.gat_bwd(_d(k["g"]), _d(k["x"]), _d(k["src"]), k["idx"], _d(k["a"]), _d(want_p))
    for n in ("gx", "da", "dbias") + (("gsrc",) if bip else ()):
        _bits(got[n], want[n], n)


# ------------------------------------------------------------------------------------------------------------------ softmax edges
@pytest.mark.parametrize("shape,bip", [((2, 5, 257, 37, 9), True), ((3, 8, 513, 513, 3), False)])
def test_softmax_is_shift_invariant_and_does_not_overflow(shape, bip):
    """bias 0, +200, -200 and NULL: the same p and agg, each within the bar of fp64 (whose four results agree to 1e-12) and within
    the sum of two bars of one another.  exp(200 + ...) without the max subtraction is inf in fp32."""
    k = R.make_case(shape, bip)
    dv = _dev(k)
    res = {}
    for name, b in (("0", 0.0), ("+200", 200.0), ("-200", -200.0), ("NULL", None)):
        bias = None if b is None else torch.tensor([b])
        agg, p, _ = _gat_fwd(dv, bias=None if bias is None else bias.cuda())
        assert _written(agg, p)
        rep = R.gat_fwd_report(f"{shape} bias {name}", agg, p, k, bias=bias)
        _held(rep, "bias " + name)
        ref = R.gat_fwd(_d(k["x"]), _d(k["src"]), k["idx"], _d(k["a"]), _d(bias))
        res[name] = (agg, p, rep, ref, R.gat_fwd_mag(_d(k["x"]), _d(k["src"]), k["idx"], _d(k["a"]), _d(bias), ref[1]))
    assert torch.equal(res["0"][0], res["NULL"][0]) and torch.equal(res["0"][1], res["NULL"][1]), "a NULL bias is a zero bias"
    for name in ("+200", "-200", "NULL"):
        (agg0, p0, rep0, ref0, _), (agg1, p1, rep1, ref1, (m_p, m_agg)) = res["0"], res[name]
        assert float((ref0[0] - ref1[0]).abs().max()) <= 1e-12 * float(ref0[0].abs().max()) and float((ref0[1] - ref1[1]).abs().max()) <= 1e-12
        assert R.rel(p1, p0, m_p) <= rep0["bound_p"] + rep1["bound_p"], name
        assert R.rel(agg1, agg0, m_agg) <= rep0["bound_agg"] + rep1["bound_agg"], name


@pytest.mark.parametrize("shape,bip", [((2, 5, 257, 37, 9), True), ((3, 8, 513, 513, 3), False)])
def test_nearly_saturated_softmax(shape, bip):
    """Logits of a row spread over up to 60 (a scaled so that the widest row has exactly that): nearly one-hot, not exactly.  The
    winners round to 1.0 while their losers, e^-60 = 8.8e-27 and more, are normal fp32 numbers that must neither vanish nor turn
    into garbage: p is held to the bar RELATIVE to itself.  (Wider rows would put losers among the fp32 denormals, where p f_n
    is no scale for anything.)"""
    k = R.make_case(shape, bip)
    e = R.gat_logits(_d(k["x"]), _d(k["src"]), k["idx"], _d(k["a"]), _d(k["bias"]))[0]
    k["a"] = k["a"] * (60.0 / float((e.max(-1).values - e.min(-1).values).max()))
    e = R.gat_logits(_d(k["x"]), _d(k["src"]), k["idx"], _d(k["a"]), _d(k["bias"]))[0]
    spread = float((e.max(-1).values - e.min(-1).values).max())
    assert 59 <= spread <= 61, spread
    dv = _dev(k)
    agg, p, p_dev = _gat_fwd(dv)
    assert _written(agg, p)
    _held(R.gat_fwd_report(f"{shape} spread {spread:.0f}", agg, p, k), "gat_fwd")
    assert bool((p > 0).all()) and int(((p.max(-1).values == 1) & (p.min(-1).values > 0)).sum()) > 0 and float(p.min()) < 1e-20
    got = _gat_bwd(dv, p_dev)
    assert _written(*got.values())
    _held(R.gat_bwd_report(f"{shape} spread {spread:.0f}", got, p, k), "gat_bwd")


@pytest.mark.parametrize("shape,bip", [((2, 5, 257, 37, 9), True), ((3, 8, 513, 513, 3), False)])
def test_nan_and_inf_reach_what_the_fp64_reference_says(shape, bip):
    """One NaN and one +inf in src (in a self graph: in x, which is the source), one NaN in x.  The NaN masks of h, p and agg (and the
    +inf mask of h) equal the fp64 reference's element for element; everything the reference has finite stays within the bar."""
    B, C, N, M, kk = shape
    k = R.make_case(shape, bip)
    s = k["src"] if bip else k["x"]
    c_up = int((k["a"][C:] > 0).nonzero()[0])                             # +inf there makes the key's logit +inf, not -inf
    s[0, 1, 11], s[B - 1, c_up, M - 1] = float("nan"), float("inf")       # key M - 1 also takes the clamped M + 7
    k["x"][B - 1, 2, 5] = float("nan")
    dv = _dev(k)
    x, src, idx, a, bias, eps = _d(k["x"]), _d(k["src"]), k["idx"], _d(k["a"]), _d(k["bias"]), _d(k["eps"])
    h, h64 = _gin_fwd(dv), R.gin_fwd(x, src, idx, eps)
    assert 0 < int(torch.isnan(h64).sum()) < h64.numel() // 2 and int((h64 == float("inf")).sum()) > 0
    assert torch.equal(torch.isnan(h), torch.isnan(h64)) and torch.equal(h == float("inf"), h64 == float("inf"))
    _held(R.gin_fwd_report(f"{shape} non-finite", h, k), "gin_fwd")
    agg, p, _ = _gat_fwd(dv)
    agg64, p64 = R.gat_fwd(x, src, idx, a, bias)
    assert 0 < int(torch.isnan(p64).sum()) < p64.numel() // 2
    assert torch.equal(torch.isnan(p), torch.isnan(p64)), (int(torch.isnan(p).sum()), int(torch.isnan(p64).sum()))
    assert torch.equal(torch.isnan(agg), torch.isnan(agg64)), (int(torch.isnan(agg).sum()), int(torch.isnan(agg64).sum()))
    assert not bool(torch.isinf(p).any()) and torch.equal(torch.isinf(agg), torch.isinf(agg64))
    _held(R.gat_fwd_report(f"{shape} non-finite", agg, p, k), "gat_fwd")


# ------------------------------------------------------------------------------------------------------------------ workspace
def _all_outputs(dv, ws_of):
    """Every output of the three workspace users, each call with the workspace ``ws_of()`` hands it."""
    agg, p, p_dev = _gat_fwd(dv, ws=ws_of())
    got = _gat_bwd(dv, p_dev, ws=ws_of())
    return [agg, p, got["gx"], got["gsrc"], got["da"], got["dbias"], *_gin_bwd(dv, ws=ws_of())]


@pytest.mark.parametrize("shape,bip", [((2, 6, 37, 257, 5), True), ((3, 8, 513, 513, 3), False), ((2, 3, 150, 1, 4), True)])
def test_dirty_workspace_gives_the_same_bits(shape, bip):
    """Exactly gkg_gconv_workspace_bytes bytes: full of 0xFF, full of zeros, and ONE buffer used by all three calls in turn."""
    dv = _dev(R.make_case(shape, bip))
    ones = _all_outputs(dv, lambda: Ws(shape, 0xFF))
    zeros = _all_outputs(dv, lambda: Ws(shape, 0x00))
    one = Ws(shape, 0x5A)
    shared = _all_outputs(dv, lambda: one)
    for a, b, c in zip(ones, zeros, shared):
        assert _written(a) and _same(a, b) and _same(a, c)


def test_one_workspace_serves_forward_backward_and_a_smaller_shape():
    big, small = (3, 8, 513, 513, 3), (2, 5, 257, 37, 9)
    ws = Ws(big)
    assert int(_L().load().gkg_gconv_workspace_bytes(*small)) < ws.n
    dv_big, dv_small = _dev(R.make_case(big, False)), _dev(R.make_case(small, True))
    first = _all_outputs(dv_big, lambda: ws)
    second = _all_outputs(dv_small, lambda: ws)                            # the layout of the small shape inside the big buffer
    for got, want in zip(first, _all_outputs(dv_big, lambda: Ws(big, 0))):
        assert _same(got, want)
    for got, want in zip(second, _all_outputs(dv_small, lambda: Ws(small, 0))):
        assert _same(got, want)


def test_a_workspace_one_byte_short_is_refused():
    lib, err_ws = _L().load(), _L()._K["ERR_WORKSPACE"]
    shape = B, C, N, M, k = (2, 5, 257, 37, 9)
    dv = _dev(R.make_case(shape, True))
    ws = Ws(shape)
    outs = dict(gx=Buf((B, C, N)), gsrc=Buf((B, C, M)), geps=Buf((1,), torch.float64), agg=Buf((B, C, N)), p=Buf((B, N, k)),
                da=Buf((2 * C,), torch.float64), db=Buf((1,), torch.float64))
    o = {n: _p(b.t) for n, b in outs.items()}
    p_in = torch.full((B, N, k), 1.0 / k, device="cuda")
    st = _st()
    assert lib.gkg_gin_bwd(_p(dv["g"]), _p(dv["x"]), _p(dv["eps"]), _p(dv["idx"]), o["gx"], o["gsrc"], o["geps"], B, C, N, M, k, _p(ws.t),
                           ws.n - 1, st) == err_ws == -4
    assert lib.gkg_gat_fwd(_p(dv["x"]), _p(dv["src"]), _p(dv["idx"]), _p(dv["a"]), _p(dv["bias"]), o["agg"], o["p"], B, C, N, M, k, _p(ws.t),
                           ws.n - 1, st) == err_ws
    assert lib.gkg_gat_bwd(_p(dv["g"]), _p(dv["x"]), _p(dv["src"]), _p(dv["idx"]), _p(dv["a"]), _p(p_in), o["gx"], o["gsrc"], o["da"], o["db"],
                           B, C, N, M, k, _p(ws.t), ws.n - 1, st) == err_ws
    assert len(lib.gkg_last_error_string()) > 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b.full).all()) for b in outs.values()), "a refused call wrote to an output"
    assert bool((ws.t == 0xFF).all()) and ws.guards_ok(), "a refused call wrote to the workspace"


# ------------------------------------------------------------------------------------------------------------------ optional outputs
@pytest.mark.parametrize("shape,bip", [((2, 5, 257, 37, 9), True), ((3, 8, 513, 513, 3), False)])
def test_optional_outputs_change_nothing_else(shape, bip):
    """geps NULL (with x NULL), da / dbias in all four combinations, bias NULL: what is written equals the all-outputs call bit for
    bit (a NULL bias: the call with a zero bias)."""
    k = R.make_case(shape, bip)
    dv = _dev(k)
    gx, gsrc, geps = _gin_bwd(dv)
    gx2, gsrc2, none = _gin_bwd(dv, geps=False)
    assert none is None and _written(gx, gsrc, geps) and _same(gx, gx2) and _same(gsrc, gsrc2)
    agg, p, p_dev = _gat_fwd(dv)
    full = _gat_bwd(dv, p_dev)
    assert _written(*full.values())
    for da, dbias in ((True, False), (False, True), (False, False)):
        part = _gat_bwd(dv, p_dev, da=da, dbias=dbias)
        assert (part["da"] is not None) == da and (part["dbias"] is not None) == dbias
        for n in ("gx", "gsrc") + (("da",) if da else ()) + (("dbias",) if dbias else ()):
            assert _same(part[n], full[n]), (n, da, dbias)
    agg0, p0, _ = _gat_fwd(dv, bias=torch.zeros(1, device="cuda"))
    aggn, pn, _ = _gat_fwd(dv, bias=None)
    assert _written(aggn, pn) and _same(agg0, aggn) and _same(p0, pn)


@pytest.mark.parametrize("shape", [R.HUB, R.FIVE_KEYS], ids=["hub", "five-keys"])
def test_two_runs_give_the_same_bits_on_long_sorted_lists(shape):
    """Hundreds of edges per key: the fill order of the lists depends on the atomics' arrival order, the sort makes it canonical."""
    dv = _dev(R.make_case(shape, True))
    r1, r2 = _all_outputs(dv, lambda: Ws(shape)), _all_outputs(dv, lambda: Ws(shape))
    for a, b in zip(r1, r2):
        assert _written(a) and _same(a, b)


# ------------------------------------------------------------------------------------------------------------------ rejections
def test_bad_arguments_are_rejected_before_any_launch():
    lib, K_ = _L().load(), _L()._K
    NULL, SHAPE = K_["ERR_NULL"], K_["ERR_SHAPE"]
    shape = B, C, N, M, k = (2, 3, 10, 7, 4)
    dv = _dev(R.make_case(shape, True))
    ws = Ws((2, 3, 10, 10, 4))                                             # also enough for the self-graph sizes below
    outs = dict(h=Buf((B, C, N)), gx=Buf((B, C, N)), gsrc=Buf((B, C, M)), geps=Buf((1,), torch.float64), agg=Buf((B, C, N)),
                p=Buf((B, N, k)), da=Buf((2 * C,), torch.float64), db=Buf((1,), torch.float64))
    p_in = torch.full((B, N, k), 1.0 / k, device="cuda")
    st = _st()
    base = dict({n: _p(b.t) for n, b in outs.items()}, g=_p(dv["g"]), x=_p(dv["x"]), src=_p(dv["src"]), idx=_p(dv["idx"]), eps=_p(dv["eps"]),
                a=_p(dv["a"]), bias=_p(dv["bias"]), pin=_p(p_in), B=B, C=C, N=N, M=M, k=k, ws=_p(ws.t), wsn=ws.n)
    order = {"gkg_gin_fwd": "x src idx eps h B C N M k",
             "gkg_gin_bwd": "g x eps idx gx gsrc geps B C N M k ws wsn",
             "gkg_gat_fwd": "x src idx a bias agg p B C N M k ws wsn",
             "gkg_gat_bwd": "g x src idx a pin gx gsrc da db B C N M k ws wsn"}
    required = {"gkg_gin_fwd": "x idx eps h", "gkg_gin_bwd": "g idx eps gx ws", "gkg_gat_fwd": "x idx a agg p ws",
                "gkg_gat_bwd": "g x idx a pin gx ws"}

    def call(fn, **kw):
        v = dict(base)
        v.update(kw)
        return getattr(lib, fn)(*[v[n] for n in order[fn].split()], st)

    def rejected(fn, code, **kw):
        rc = call(fn, **kw)
        assert rc == code, (fn, kw, rc)
        assert len(lib.gkg_last_error_string()) > 0, (fn, kw, "no error string")

    for fn in order:
        for name in required[fn].split():
            rejected(fn, NULL, **{name: None})
        for dim in "BCNMk":
            rejected(fn, SHAPE, **{dim: 0})
            rejected(fn, SHAPE, **{dim: -3})
        rejected(fn, SHAPE, B=65536)
        rejected(fn, SHAPE, C=65536)
    # a self graph (no src / gsrc) needs M == N
    rejected("gkg_gin_fwd", SHAPE, src=None)
    rejected("gkg_gin_bwd", SHAPE, gsrc=None)
    rejected("gkg_gat_fwd", SHAPE, src=None)
    rejected("gkg_gat_bwd", SHAPE, src=None, gsrc=None)
    # src and gsrc come together; geps needs x
    rejected("gkg_gat_bwd", NULL, gsrc=None)
    rejected("gkg_gat_bwd", NULL, src=None)
    rejected("gkg_gat_bwd", NULL, src=None, M=N)
    rejected("gkg_gin_bwd", NULL, x=None)
    assert lib.gkg_gconv_workspace_bytes(B, C, N, 0, k) == 0 and lib.gkg_gconv_workspace_bytes(B, C, N, M, -1) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b.full).all()) for b in outs.values()), "a rejected call wrote to an output"
    assert bool((ws.t == 0xFF).all()) and ws.guards_ok(), "a rejected call wrote to the workspace"
    # the same arguments, unmodified, are accepted, and so are the optional ones left out
    for fn in order:
        assert call(fn) == 0, fn
    assert call("gkg_gin_bwd", x=None, geps=None) == 0 and call("gkg_gat_fwd", bias=None) == 0 and call("gkg_gat_bwd", da=None, db=None) == 0
    assert call("gkg_gin_fwd", src=None, M=N) == 0 and call("gkg_gat_bwd", src=None, gsrc=None, M=N) == 0
    torch.cuda.synchronize()
    assert all(b.guards_ok() for b in outs.values()) and ws.guards_ok()


# ------------------------------------------------------------------------------------------------------------------ bounded random pass
def test_thirty_random_problems():
    rng = random.Random(20250314)
    for i in range(30):
        B, C, M, kk = rng.randint(1, 3), rng.randint(1, 24), rng.randint(1, 600), rng.randint(1, 20)
        bip = rng.random() < 0.6
        N = rng.randint(1, min(600, max(1, 800 * M // kk))) if bip else M      # at most ~800 edges into one key: the sort is quadratic
        shape = (B, C, N, M, kk)
        k = R.make_case(shape, bip, seed=7000 + i)
        if rng.random() < 0.3:
            k["bias"] = None
        want_geps, want_da, want_db = rng.random() < 0.5, rng.random() < 0.5, rng.random() < 0.5
        tag = f"random #{i} {shape} {'bipartite' if bip else 'self'}"
        dv = _dev(k)
        _held(R.gin_fwd_report(tag, _gin_fwd(dv), k), tag)
        gx, gsrc, geps = _gin_bwd(dv, geps=want_geps)
        assert _written(gx, gsrc, geps)
        _held(R.gin_bwd_report(tag, gx, gsrc, geps, k), tag)
        agg, p, p_dev = _gat_fwd(dv)
        assert _written(agg, p)
        _held(R.gat_fwd_report(tag, agg, p, k), tag)
        got = _gat_bwd(dv, p_dev, da=want_da, dbias=want_db)
        assert _written(*got.values())
        _held(R.gat_bwd_report(tag, got, p, k), tag)
