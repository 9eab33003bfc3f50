"""tests/gconv_ref.py — the fp64 reference the GPU tests hold csrc/gkg_gconv.hip to — pinned on the CPU, in double.

AGAINST AUTOGRAD.  The literal form of the reference (gather to (B, C, N, k); GIN: (1 + eps) x + sum over k; graph attention:
logits from the two halves of ``a`` and the bias, softmax(-1), the weighted sum) is differentiated by torch in double; gconv_ref's
gin_fwd / gin_bwd / gat_fwd / gat_bwd must give the same h, agg, gx, gsrc, geps, da and dbias to 1e-11 at every shape of the GPU
tests, self graph and bipartite.  Central differences along random directions pin gx and gsrc a second time, without autograd.

SENSITIVITY.  Seventeen wrong formulas are evaluated in double and put through the very report functions and bound constants the
GPU tests use, on the GPU tests' own inputs: each must land above the bar on at least one listed shape (the test prints which),
or the bar could not tell it from the right formula.  "No bias" and "no t[n] = a[:C] . x[n]" are NOT among them: the softmax is
shift-invariant and both are constant over k, so dropping them changes no output (their gradients da[:C] and dbias are exactly 0,
which the scales of gconv_ref judge absolutely).

EXACT FAMILIES.  The three families the GPU file compares bit for bit are exact in plain fp32 on the CPU as well."""
import pytest
import torch
import torch.nn.functional as F

import gconv_ref as R

d = lambda t: None if t is None else t.double()                              # noqa: E731


def _close(a, b, tol=1e-11):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _gather64(src, idx):
    """The literal gather of tests/test_hip_gconv.py."""
    B, C, M = src.shape
    N, k = idx.shape[1:]
    j = idx.clamp(0, M - 1)
    return torch.gather(src, 2, j.reshape(B, 1, N * k).expand(B, C, N * k)).reshape(B, C, N, k)


def _literal_gin(x, src, idx, eps):
    return (1 + eps) * x + _gather64(x if src is None else src, idx).sum(-1)


def _literal_gat(x, src, idx, a, bias):
    C = x.shape[1]
    xj = _gather64(x if src is None else src, idx)
    e = torch.einsum("c,bcn->bn", a[:C], x)[..., None] + torch.einsum("c,bcnk->bnk", a[C:], xj)
    if bias is not None:
        e = e + bias
    p = torch.softmax(e, -1)
    return (p[:, None] * xj).sum(-1), p


# ------------------------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("shape,bip", R.CASES, ids=R.IDS)
def test_reference_matches_autograd_of_the_literal_form(shape, bip):
    k = R.make_case(shape, bip)
    B, C, N, M, kk = shape
    idx, g = k["idx"], d(k["g"])
    leaf = lambda t: None if t is None else t.double().requires_grad_(True)    # noqa: E731
    # ---- GIN
    x, src, eps = leaf(k["x"]), leaf(k["src"]), leaf(k["eps"])
    want = _literal_gin(x, src, idx, eps)
    want.backward(g)
    with torch.no_grad():
        assert _close(R.gin_fwd(x, src, idx, eps), want), "h"
        gx, gsrc, geps = R.gin_bwd(g, x, eps, idx, M, bip)
    assert _close(gx, x.grad), "gin gx"
    assert (gsrc is None) == (not bip) and (gsrc is None or _close(gsrc, src.grad)), "gin gsrc"
    assert _close(geps, eps.grad.reshape(())), "geps"
    # ---- graph attention, with and without a bias
    for with_bias in (True, False):
        x, src, a, bias = leaf(k["x"]), leaf(k["src"]), leaf(k["a"]), (leaf(k["bias"]) if with_bias else None)
        want, want_p = _literal_gat(x, src, idx, a, bias)
        want.backward(g)
        with torch.no_grad():
            agg, p = R.gat_fwd(x, src, idx, a, bias)
            assert _close(agg, want) and _close(p, want_p), "agg / p"
            got = R.gat_bwd(g, x, src, idx, a, p)
        assert _close(got["gx"], x.grad), "gat gx"
        assert (got["gsrc"] is None) == (not bip) and (got["gsrc"] is None or _close(got["gsrc"], src.grad)), "gat gsrc"
        assert _close(got["da"], a.grad), "da"
        assert float(a.grad[:C].abs().max()) <= 1e-11 * max(1.0, float(a.grad.abs().max())), "da[:C] is 0 in exact arithmetic"
        if with_bias:
            assert _close(got["dbias"], bias.grad.reshape(())) and abs(float(bias.grad)) <= 1e-11 * max(1.0, float(a.grad.abs().max()))


@pytest.mark.parametrize("shape,bip", [((2, 5, 33, 11, 4), True), ((2, 5, 33, 33, 4), False), ((1, 3, 9, 1, 2), True)])
def test_projected_gradients_pin_gsrc_and_gx_directly(shape, bip):
    """<gx, vx> + <gsrc, vs> against the central difference of <out, g> along (vx, vs), in double: no autograd involved."""
    k = R.make_case(shape, bip, seed=91)
    gen = torch.Generator().manual_seed(92)
    x, src, idx, a, bias, eps, g = d(k["x"]), d(k["src"]), k["idx"], d(k["a"]), d(k["bias"]), d(k["eps"]), d(k["g"])
    M, h = shape[3], 1e-6
    for turn in range(3):
        vx = torch.randn(x.shape, generator=gen, dtype=torch.float64) * (turn != 1)     # turn 1: src alone, turn 2: x alone
        vs = None if src is None else torch.randn(src.shape, generator=gen, dtype=torch.float64) * (turn != 2)
        sh = lambda s: (x + s * h * vx, None if src is None else src + s * h * vs)     # noqa: E731
        gx, gsrc, _ = R.gin_bwd(g, x, eps, idx, M, bip)
        num = ((R.gin_fwd(*sh(1), idx, eps) - R.gin_fwd(*sh(-1), idx, eps)) * g).sum() / (2 * h)
        ana = (gx * vx).sum() + (0 if gsrc is None else (gsrc * vs).sum())
        assert abs(float(num - ana)) <= 1e-7 * max(1.0, abs(float(ana))), ("gin", turn, float(num), float(ana))
        p = R.gat_fwd(x, src, idx, a, bias)[1]
        got = R.gat_bwd(g, x, src, idx, a, p)
        num = ((R.gat_fwd(*sh(1), idx, a, bias)[0] - R.gat_fwd(*sh(-1), idx, a, bias)[0]) * g).sum() / (2 * h)
        ana = (got["gx"] * vx).sum() + (0 if got["gsrc"] is None else (got["gsrc"] * vs).sum())
        assert abs(float(num - ana)) <= 1e-7 * max(1.0, abs(float(ana))), ("gat", turn, float(num), float(ana))


def test_clamp_softmax_and_scatter_rules():
    assert R.clamp(torch.tensor([-5, 0, 3, 4, 11]), 4).tolist() == [0, 0, 3, 3, 3]
    e = torch.tensor([[1000.0, 999.0], [-1000.0, -1000.0], [0.0, float("nan")], [float("inf"), 0.0]], dtype=torch.float64)
    p = R.softmax(e)
    assert _close(p[:2], torch.softmax(e[:2], -1)) and bool(torch.isnan(p[2:]).all())
    v = torch.arange(6.0).view(1, 1, 2, 3)
    assert R.scatter(v, torch.tensor([[[0, 0, 9], [-1, 1, 2]]]), 3).tolist() == [[[4.0, 4.0, 7.0]]]


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def _gat_bwd_variant(g, x, src, idx, a, p, de_no_dot=False, dot_no_p=False, no_de_term=False, a1_in_gsrc=False, da_from_x=False):
    """gconv_ref.gat_bwd with one term wrong."""
    B, C, N = x.shape
    s = x if src is None else src
    M = s.shape[2]
    dp = R.csum(g.unsqueeze(-1) * R.gather(s, idx))
    dot = R.ksum(dp if dot_no_p else p * dp).unsqueeze(-1)
    de = p * dp if de_no_dot else p * (dp - dot)
    sde = R.ksum(de)
    a2 = a[:C] if a1_in_gsrc else a[C:]
    sc = R.scatter(p.unsqueeze(1) * g.unsqueeze(-1) + (0 if no_de_term else de.unsqueeze(1) * a2.view(1, C, 1, 1)), idx, M)
    gx = sde.unsqueeze(1) * a[:C].view(1, C, 1)
    key = (sde.unsqueeze(1) * x) if da_from_x else (R.scatter_e(de, idx, M).unsqueeze(1) * s)
    da = torch.cat([(sde.unsqueeze(1) * x).sum(dim=(0, 2)), key.sum(dim=(0, 2))])
    return dict(gx=gx if src is not None else gx + sc, gsrc=sc if src is not None else None, da=da, dbias=sde.sum())


def _gin_mutants(k):
    """name -> report of the wrong formula, or None where the formula does not differ by construction (k = 1, B = 1, ...)."""
    B, C, N, M, kk = k["shape"]
    x, src, idx, eps, g = d(k["x"]), d(k["src"]), k["idx"], d(k["eps"]), d(k["g"])
    bip = src is not None
    s = x if src is None else src
    fwd = lambda h: R.gin_fwd_report("", h, k)                                   # noqa: E731
    bwd = lambda gx, gsrc, geps: R.gin_bwd_report("", gx, gsrc, geps, k)         # noqa: E731
    gx, gsrc, geps = R.gin_bwd(g, x, eps, idx, M, bip)
    sc = gsrc if bip else gx - (1 + eps) * g
    both = lambda gx_part, sc_: (gx_part, sc_) if bip else (gx_part + sc_, None)  # noqa: E731
    xj = R.gather(s, idx)
    roll = idx.roll(-1, 0)
    out = {
        "eps for 1 + eps": fwd(eps * x + R.ksum(xj)),
        "mean for sum": fwd((1 + eps) * x + R.ksum(xj) / kk) if kk > 1 else None,
        "last neighbour dropped": fwd((1 + eps) * x + R.ksum(xj[..., :-1])) if kk > 1 else fwd((1 + eps) * x),
        "index + 1": fwd(R.gin_fwd(x, src, idx + 1, eps)),
        "index + 1 (transposed graph)": bwd(*R.gin_bwd(g, x, eps, idx + 1, M, bip)),
        "self term missing in the self-graph backward": None if bip else bwd(sc, None, geps),
        "gsrc scaled by 1 + eps": bwd(*both((1 + eps) * g, (1 + eps) * sc), geps),
        "geps = sum gh": bwd(gx, gsrc, g.sum()),
        "lists of image (b + 1) mod B": fwd(R.gin_fwd(x, src, roll, eps)) if B > 1 else None,
        "lists of image (b + 1) mod B (transposed graph)": bwd(*R.gin_bwd(g, x, eps, roll, M, bip)) if B > 1 else None,
    }
    assert R.passes(fwd(R.gin_fwd(x, src, idx, eps))) and R.passes(bwd(gx, gsrc, geps)), "the right formula"
    return out


def _gat_mutants(k):
    B, C, N, M, kk = k["shape"]
    x, src, idx, a, bias, g = d(k["x"]), d(k["src"]), k["idx"], d(k["a"]), d(k["bias"]), d(k["g"])
    s = x if src is None else src
    fwd = lambda agg, p: R.gat_fwd_report("", agg, p, k)                         # noqa: E731
    e, _ = R.gat_logits(x, src, idx, a, bias)
    agg, p = R.gat_fwd(x, src, idx, a, bias)
    p32 = p.float()                                                              # the p the backward is given, as at the ABI
    bwd = lambda **kw: R.gat_bwd_report("", _gat_bwd_variant(g, x, src, idx, a, d(p32), **kw), p32, k)   # noqa: E731
    xj = R.gather(s, idx)
    weigh = lambda q: R.ksum(q.unsqueeze(1) * xj)                                # noqa: E731
    p_leaky = R.softmax(F.leaky_relu(e, 0.1))
    p_swap = R.gat_fwd(x, src, idx, torch.cat([a[C:], a[:C]]), bias)[1]
    p_raw = torch.exp(e - e.max(dim=-1, keepdim=True).values)
    out = {
        "LeakyReLU on the logits": fwd(weigh(p_leaky), p_leaky),
        "a halves swapped": fwd(weigh(p_swap), p_swap),
        "p not normalised": fwd(weigh(p_raw), p_raw),
        "p of neighbour k + 1": fwd(weigh(p.roll(-1, -1)), p) if kk > 1 else None,
        "de without - sum p dp": bwd(de_no_dot=True),
        "dot without p": bwd(dot_no_p=True) if kk > 1 else None,
        "gsrc without the de a[C:] term": bwd(no_de_term=True),
        "gsrc using a[:C]": bwd(a1_in_gsrc=True),
        "da[C:] from x instead of src[j]": bwd(da_from_x=True),
    }
    assert R.passes(fwd(agg, p)) and R.passes(bwd()), "the right formula"
    return out


GIN_MUTANTS = ["eps for 1 + eps", "mean for sum", "last neighbour dropped", "index + 1", "index + 1 (transposed graph)",
               "self term missing in the self-graph backward", "gsrc scaled by 1 + eps", "geps = sum gh",
               "lists of image (b + 1) mod B", "lists of image (b + 1) mod B (transposed graph)"]
GAT_MUTANTS = ["LeakyReLU on the logits", "a halves swapped", "p not normalised", "p of neighbour k + 1", "de without - sum p dp",
               "dot without p", "gsrc without the de a[C:] term", "gsrc using a[:C]", "da[C:] from x instead of src[j]"]
_reports = {}


def _all_reports(kind):
    """{case id: {mutant: report}}, computed once per operator and shared by the parametrised cases below."""
    if kind not in _reports:
        make = _gin_mutants if kind == "gin" else _gat_mutants
        _reports[kind] = {i: make(R.make_case(s, b)) for (s, b), i in zip(R.CASES, R.IDS)}
    return _reports[kind]


@pytest.mark.parametrize("kind,name", [("gin", n) for n in GIN_MUTANTS] + [("gat", n) for n in GAT_MUTANTS])
def test_each_wrong_formula_lands_above_the_bar_of_the_gpu_tests(kind, name):
    reps = _all_reports(kind)
    assert set(next(iter(reps.values()))) == set(GIN_MUTANTS if kind == "gin" else GAT_MUTANTS)
    above = [i for i, r in reps.items() if r[name] is not None and not R.passes(r[name])]
    tried = [i for i, r in reps.items() if r[name] is not None]
    print(f"\n{kind}: '{name}' lands above the bar at {len(above)} of {len(tried)} cases: {', '.join(above)}")
    assert above, (kind, name, "the bar cannot tell this formula from the right one at any listed shape")
    # every shape with more than one edge per row and more than one key sees it (the degenerate shapes cannot: k = 1, M = 1)
    general = [i for (s, b), i in zip(R.CASES, R.IDS) if i in tried and s[3] > 1 and s[4] > 1]
    assert set(general) <= set(above), (kind, name, sorted(set(general) - set(above)))


# ------------------------------------------------------------------------------------------------------------------ exact families
def _same_bits(a, b):
    return a.dtype == torch.float32 and torch.equal(a.double(), b)


@pytest.mark.parametrize("shape,bip", R.CASES, ids=R.IDS)
def test_gin_on_the_quarter_grid_is_exact_in_fp32(shape, bip):
    k = R.make_exact_case(shape, bip)
    M = shape[3]
    x, src, idx, eps, g = (k[n] for n in ("x", "src", "idx", "eps", "g"))
    assert _same_bits(R.gin_fwd(x, src, idx, eps), R.gin_fwd(d(x), d(src), idx, d(eps)))
    got, want = R.gin_bwd(g, x, eps, idx, M, bip), R.gin_bwd(d(g), d(x), d(eps), idx, M, bip)
    assert _same_bits(got[0], want[0]) and (not bip or _same_bits(got[1], want[1]))
    gh = ((torch.arange(shape[1]).view(1, -1, 1) + 1) * (torch.arange(shape[2]).view(1, 1, -1) + 1)).float().expand(shape[0], -1, -1)
    got, want = R.gin_bwd(gh, x, eps, idx, M, bip), R.gin_bwd(d(gh), d(x), d(eps), idx, M, bip)
    assert _same_bits(got[0], want[0]) and (not bip or _same_bits(got[1], want[1]))


@pytest.mark.parametrize("shape,bip", R.UNIFORM_SHAPES)
def test_gat_with_zero_weights_is_exact_in_fp32(shape, bip):
    """a = 0, k a power of two: p = 1 / k; agg, de, gsrc, da[C:] exact, sde (hence gx on a bipartite graph, da[:C], dbias) 0."""
    k = R.make_exact_case(shape, bip)
    C, kk = shape[1], shape[4]
    x, src, idx, a, bias, g = (k[n] for n in ("x", "src", "idx", "a", "bias", "g"))
    agg, p = R.gat_fwd(x, src, idx, a, bias)
    agg64, p64 = R.gat_fwd(d(x), d(src), idx, d(a), d(bias))
    assert bool((p == 1.0 / kk).all()) and _same_bits(p, p64) and _same_bits(agg, agg64)
    got, want = R.gat_bwd(g, x, src, idx, a, p), R.gat_bwd(d(g), d(x), d(src), idx, d(a), p64)
    for n in ("de", "gx", "da", "dbias") + (("gsrc",) if bip else ()):
        assert _same_bits(got[n], want[n]), n
    assert bool((got["sde"] == 0).all()) and float(got["dbias"]) == 0 and bool((got["da"][:C] == 0).all())
    assert float(got["da"][C:].abs().max()) > 0 and (not bip or bool((got["gx"] == 0).all()))


@pytest.mark.parametrize("shape,bip", R.ONE_HOT_SHAPES)
def test_key_score_of_128_makes_fp32_softmax_exactly_one_hot(shape, bip):
    k = R.make_one_hot_case(shape, bip)
    x, src, idx, a, bias, g = (k[n] for n in ("x", "src", "idx", "a", "bias", "g"))
    agg, p = R.gat_fwd(x, src, idx, a, bias)
    want_p, want_agg = R.one_hot_expect(k)
    assert torch.equal(p, want_p) and torch.equal(agg, want_agg)
    p64 = R.gat_fwd(d(x), d(src), idx, d(a), d(bias))[1]
    score = R.gather((x if src is None else src)[:, :1], idx).squeeze(1).sort(-1).values
    if float((score[..., -1] - score[..., -2]).min()) * 128 < 700:               # e^-745 is 0 in double as well
        assert not torch.equal(p64, d(want_p)), "the fp64 softmax is not one-hot: the expectation is the gather, not fp64"
    got, want = R.gat_bwd(g, x, src, idx, a, p), R.gat_bwd(d(g), d(x), d(src), idx, d(a), d(p))
    for n in ("gx", "da", "dbias") + (("gsrc",) if bip else ()):
        assert _same_bits(got[n], want[n]), n
