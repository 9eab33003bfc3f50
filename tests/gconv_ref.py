"""Plain torch restatement of what include/gkg_hip.h promises for the GIN and graph-attention aggregations (csrc/gkg_gconv.hip, the
"GIN and graph-attention aggregations" block of the header): gkg_gin_fwd, gkg_gin_bwd, gkg_gat_fwd, gkg_gat_bwd.

Every function computes in the dtype of its inputs.  Called with ``.double()`` operands it is the REFERENCE the GPU tests hold the
kernels to; called with the fp32 operands themselves it is the YARDSTICK: the error an honest fp32 implementation of the same
formula makes against the fp64 reference ("plain fp32": one accumulator, left to right, for every sum over k, over the channels
and over the edges of a key; torch.sum's cascade summation is more accurate than that).  tests/test_gconv_reference_host.py pins
these formulas to torch autograd of the literal form (gather to (B, C, N, k), softmax(-1), sums) in double on the CPU and shows
that the bar below tells each of a list of wrong formulas from the right one.

Shapes: x / g / gh (B, C, N), src (B, C, M) or None (self graph: src = x, M == N), idx (B, N, k) int64 (clamped into [0, M)),
a (2 C), bias / eps (1,) (bias may be None), p / de (B, N, k).  ``gat_bwd`` takes p as an INPUT, as the entry point does.

The module also holds what the GPU file and the host file must share so that they cannot drift: the bound constants (edge_ref's),
the scales, the report functions, the shape list and the input generators.  A helper module, not a test module and not a conftest."""
import torch

from edge_ref import FLOOR, K, SUM_TOL, _flat, bound, clamp, gather          # noqa: F401  (the bar is edge_ref's, re-exported)

# (B, C, N, M, k): see tests/test_hip_gconv_fp64.py for what each one is there for
SHAPES = [(1, 1, 1, 1, 1), (2, 5, 255, 37, 9), (2, 5, 256, 37, 9), (2, 5, 257, 37, 9), (2, 6, 37, 257, 5), (1, 4, 40, 700, 3),
          (3, 8, 513, 513, 3), (1, 20, 300, 5, 4), (2, 3, 150, 1, 4), (2, 12, 64, 600, 64), (4, 3, 70, 1000, 6)]
# (shape, bipartite): every shape with a distinct src buffer, and the self graph (src NULL) wherever M == N
CASES = [(s, True) for s in SHAPES] + [(s, False) for s in SHAPES if s[2] == s[3]]
IDS = ["x".join(map(str, s)) + ("-bip" if b else "-self") for s, b in CASES]
HUB, FIVE_KEYS = (2, 3, 150, 1, 4), (1, 20, 300, 5, 4)


# ------------------------------------------------------------------------------------------------------------------ sums
def ksum(t):
    """Sum over the last dimension, one accumulator, left to right."""
    acc = torch.zeros_like(t[..., 0])
    for kk in range(t.shape[-1]):
        acc = acc + t[..., kk]
    return acc


def csum(t):
    """Sum over dimension 1 (the channels), one accumulator, in channel order."""
    acc = torch.zeros_like(t[:, 0])
    for c in range(t.shape[1]):
        acc = acc + t[:, c]
    return acc


def scatter(v, idx, M):
    """Per-edge v (B, C, N, k) -> (B, C, M): index_add_ over the clamped indices (edge order, one accumulator per key)."""
    B, C, N, k = v.shape
    out = torch.zeros(B * C * M, dtype=v.dtype)
    out.index_add_(0, _flat(idx, B, C, M).reshape(-1), v.reshape(-1))
    return out.view(B, C, M)


def scatter_e(v, idx, M):
    """Per-edge v (B, N, k) -> (B, M)."""
    return scatter(v.unsqueeze(1), idx, M).squeeze(1)


def _src(x, src):
    return x if src is None else src


# ------------------------------------------------------------------------------------------------------------------ GIN
def gin_fwd(x, src, idx, eps):
    """gkg_gin_fwd: h = (1 + eps) x + sum_k src[j]."""
    return (1 + eps) * x + ksum(gather(_src(x, src), idx))


def gin_fwd_mag(x, src, idx, eps):
    return ((1 + eps) * x).abs() + ksum(gather(_src(x, src), idx).abs())


def gin_bwd(gh, x, eps, idx, M, bipartite):
    """gkg_gin_bwd -> (gx, gsrc or None, geps).  gx = (1 + eps) gh; gsrc[j] += gh[n] over every edge (self graph: into gx);
    geps = sum gh x."""
    k = idx.shape[2]
    sc = scatter(gh.unsqueeze(-1).expand(-1, -1, -1, k), idx, M)
    gx = (1 + eps) * gh
    return (gx, sc, (gh * x).sum()) if bipartite else (gx + sc, None, (gh * x).sum())


def gin_bwd_mag(gh, x, eps, idx, M, bipartite):
    gx, gsrc, _ = gin_bwd(gh.abs(), x, eps.abs(), idx, M, bipartite)          # 1 + |eps| >= |1 + eps|
    return gx, gsrc, (gh * x).abs().sum()


# ------------------------------------------------------------------------------------------------------------------ GAT
def gat_logits(x, src, idx, a, bias):
    """e[b][n][k] = a[:C] . x[n] + bias + a[C:] . src[j] -> (e (B, N, k), f (B, N) = 1 + 2 max_k of the logit's term magnitudes)."""
    C = x.shape[1]
    s = _src(x, src)
    a1, a2 = a[:C].view(1, C, 1), a[C:].view(1, C, 1)
    t = csum(a1 * x)
    t = t if bias is None else t + bias
    e = t.unsqueeze(-1) + gather(csum(a2 * s).unsqueeze(1), idx).squeeze(1)
    L = csum((a1 * x).abs()).unsqueeze(-1) + gather(csum((a2 * s).abs()).unsqueeze(1), idx).squeeze(1)
    L = L if bias is None else L + bias.abs()
    return e, 1 + 2 * L.max(dim=-1).values


def softmax(e):
    """Max-subtracted softmax over k.  A NaN or +inf logit makes its whole row NaN, as in torch.softmax."""
    v = torch.exp(e - e.max(dim=-1, keepdim=True).values)
    return v / ksum(v).unsqueeze(-1)


def gat_fwd(x, src, idx, a, bias):
    """gkg_gat_fwd -> (agg (B, C, N), p (B, N, k))."""
    p = softmax(gat_logits(x, src, idx, a, bias)[0])
    return ksum(p.unsqueeze(1) * gather(_src(x, src), idx)), p


def gat_fwd_mag(x, src, idx, a, bias, p):
    """(scale of p, scale of agg): p f_n and sum_k p |src_j| f_n."""
    f = gat_logits(x, src, idx, a, bias)[1]
    return p * f.unsqueeze(-1), ksum(p.unsqueeze(1) * gather(_src(x, src), idx).abs()) * f.unsqueeze(1)


def gat_de(g, x, src, idx, p):
    """dp = g[n] . src[j], de = p (dp - sum_k p dp) -> (de, sde = sum_k de), (B, N, k) and (B, N)."""
    dp = csum(g.unsqueeze(-1) * gather(_src(x, src), idx))
    de = p * (dp - ksum(p * dp).unsqueeze(-1))
    return de, ksum(de)


def gat_bwd(g, x, src, idx, a, p):
    """gkg_gat_bwd -> dict(gx, gsrc (None for a self graph), da (2 C), dbias, de, sde).  gsrc[j] += p g[n] + de a[C:]; gx[n] =
    (sum_k de) a[:C] (+ the scatter for a self graph); da = [sum (sum_k de) x[n], sum de src[j]]; dbias = sum de."""
    B, C, N = x.shape
    s = _src(x, src)
    M = s.shape[2]
    de, sde = gat_de(g, x, src, idx, p)
    sc = scatter(p.unsqueeze(1) * g.unsqueeze(-1) + de.unsqueeze(1) * a[C:].view(1, C, 1, 1), idx, M)
    gx = sde.unsqueeze(1) * a[:C].view(1, C, 1)
    da = torch.cat([(sde.unsqueeze(1) * x).sum(dim=(0, 2)), (scatter_e(de, idx, M).unsqueeze(1) * s).sum(dim=(0, 2))])
    return dict(gx=gx if src is not None else gx + sc, gsrc=sc if src is not None else None, da=da, dbias=sde.sum(), de=de, sde=sde)


def gat_bwd_mag(g, x, src, idx, a, bias, p):
    """The scales of gat_bwd's results: D = sum_c |g src_j|, demag = p (D + sum_k p D) f_n per edge, then the same sums with
    every factor replaced by its magnitude."""
    B, C, N = x.shape
    s = _src(x, src)
    M = s.shape[2]
    f = gat_logits(x, src, idx, a, bias)[1]
    p = p.abs()
    D = csum((g.unsqueeze(-1) * gather(s, idx)).abs())
    demag = p * (D + ksum(p * D).unsqueeze(-1)) * f.unsqueeze(-1)
    sdemag = ksum(demag)
    sc = scatter((p * f.unsqueeze(-1)).unsqueeze(1) * g.abs().unsqueeze(-1) + demag.unsqueeze(1) * a[C:].abs().view(1, C, 1, 1), idx, M)
    gx = sdemag.unsqueeze(1) * a[:C].abs().view(1, C, 1)
    da = torch.cat([(sdemag.unsqueeze(1) * x.abs()).sum(dim=(0, 2)), (scatter_e(demag, idx, M).unsqueeze(1) * s.abs()).sum(dim=(0, 2))])
    return dict(gx=gx if src is not None else gx + sc, gsrc=sc if src is not None else None, da=da, dbias=sdemag.sum(), de=demag,
                sde=sdemag)


# ------------------------------------------------------------------------------------------------------------------ error measure
def rel(got, ref, scale):
    """max |got - ref| / scale in double over the elements whose reference and scale are finite (0 where both the scale and the
    difference vanish; a non-finite ``got`` where the reference is finite counts as infinite)."""
    got, ref, scale = (torch.as_tensor(t).double().reshape(-1) for t in (got, ref, scale))
    ok = torch.isfinite(ref) & torch.isfinite(scale)
    if not bool(ok.any()):
        return 0.0
    d = (got[ok] - ref[ok]).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    return float((d / scale[ok].clamp_min(1e-300)).max())


def _d(t):
    return None if t is None else t.double()


def _line(tag, rep, names):
    if not tag:                                                                  # the host file's sensitivity pass: hundreds of reports
        return
    parts = [f"{n} yardstick {rep['yard_' + n]:.3e} got {rep[n]:.3e} bound {rep['bound_' + n]:.3e}" for n in names if rep.get(n) is not None]
    print(f"GCONV {tag}: " + "; ".join(parts))


def _entry(rep, name, got, yard, ref, scale, fixed=None):
    """One result of a report: its error, the yardstick's and the bound (``fixed``: SUM_TOL instead of the fp32 bar)."""
    y = rel(yard, ref, scale)
    rep["yard_" + name] = y
    rep["bound_" + name] = fixed if fixed is not None else bound(y)
    rep[name] = None if got is None else rel(got, ref, scale)


def passes(rep):
    """Every measured figure of a report is within its bound."""
    return all(rep[n[6:]] <= v for n, v in rep.items() if n.startswith("bound_") and rep[n[6:]] is not None)


# ------------------------------------------------------------------------------------------------------------------ reports
# Each takes the results to be judged (CPU tensors of any dtype; None: not produced) and the fp32 operands of the case ``k`` (a
# dict of make_case), prints one line of figures under ``tag`` and returns dict(<name>, yard_<name>, bound_<name>).
def gin_fwd_report(tag, h, k):
    x, src, idx, eps = k["x"], k["src"], k["idx"], k["eps"]
    rep = {}
    _entry(rep, "h", h, gin_fwd(x, src, idx, eps), gin_fwd(_d(x), _d(src), idx, _d(eps)), gin_fwd_mag(_d(x), _d(src), idx, _d(eps)))
    _line(tag and tag + " gin_fwd", rep, ["h"])
    return rep


def gin_bwd_report(tag, gx, gsrc, geps, k):
    """geps is an fp64 sum of exact products: SUM_TOL of the sum of |gh x| (its yardstick figure is the fp32 sum's, for the record)."""
    x, idx, eps, gh = k["x"], k["idx"], k["eps"], k["g"]
    bip, M = k["src"] is not None, k["shape"][3]
    r_x, r_s, r_e = gin_bwd(_d(gh), _d(x), _d(eps), idx, M, bip)
    m_x, m_s, m_e = gin_bwd_mag(_d(gh), _d(x), _d(eps), idx, M, bip)
    y_x, y_s, y_e = gin_bwd(gh, x, eps, idx, M, bip)
    rep = {}
    _entry(rep, "gx", gx, y_x, r_x, m_x)
    if bip:
        _entry(rep, "gsrc", gsrc, y_s, r_s, m_s)
    _entry(rep, "geps", geps, y_e, r_e, m_e, fixed=SUM_TOL)
    _line(tag and tag + " gin_bwd", rep, ["gx", "gsrc", "geps"])
    return rep


def gat_fwd_report(tag, agg, p, k, bias="case"):
    """``bias``: the bias the results were computed with (default: the case's own)."""
    x, src, idx, a = k["x"], k["src"], k["idx"], k["a"]
    bias = k["bias"] if isinstance(bias, str) else bias
    r_agg, r_p = gat_fwd(_d(x), _d(src), idx, _d(a), _d(bias))
    y_agg, y_p = gat_fwd(x, src, idx, a, bias)
    m_p, m_agg = gat_fwd_mag(_d(x), _d(src), idx, _d(a), _d(bias), r_p)
    rep = {}
    _entry(rep, "p", p, y_p, r_p, m_p)
    _entry(rep, "agg", agg, y_agg, r_agg, m_agg)
    _line(tag and tag + " gat_fwd", rep, ["p", "agg"])
    return rep


def gat_bwd_report(tag, got, p, k, names=("gx", "gsrc", "da", "dbias")):
    """``got``: dict with any of gx, gsrc, da, dbias (and de, sde for the host tests); ``p``: the fp32 p the backward was given."""
    x, src, idx, a, bias, g = k["x"], k["src"], k["idx"], k["a"], k["bias"], k["g"]
    ref = gat_bwd(_d(g), _d(x), _d(src), idx, _d(a), _d(p))
    mag = gat_bwd_mag(_d(g), _d(x), _d(src), idx, _d(a), _d(bias), _d(p))
    yard = gat_bwd(g, x, src, idx, a, p)
    rep = {}
    for n in names:
        if ref[n] is not None:
            _entry(rep, n, got.get(n), yard[n], ref[n], mag[n])
    _line(tag and tag + " gat_bwd", rep, names)
    return rep


# ------------------------------------------------------------------------------------------------------------------ inputs
def random_graph(B, N, M, k, gen):
    """randint lists (repeats are natural), every third row repeating its first neighbour, two out-of-range entries (-5 and
    M + 7: keys 0 and M - 1), different lists per image."""
    idx = torch.randint(0, M, (B, N, k), generator=gen)
    if k >= 2:
        idx[:, ::3, 1] = idx[:, ::3, 0]
    idx[0, 0, 0], idx[-1, -1, -1] = -5, M + 7
    return idx


def distinct_graph(B, N, M, k, gen):
    """Rows without a repeated key (k <= M)."""
    return torch.rand(B, N, M, generator=gen).argsort(-1)[..., :k].contiguous()


def case_seed(shape, bipartite):
    return 2003 + sum(shape) + int(bipartite)


def make_case(shape, bipartite, seed=None):
    """fp32 CPU operands of one problem: x, src with per-channel offsets of up to one standard deviation (so the sums see
    cancellation), a ~ N(0, 2.25 / C) (logits of a row spread over a few units: neither uniform nor saturated), bias 0.3,
    eps 0.3, g ~ N(0.5, 1) (the upstream gradient of both operators)."""
    B, C, N, M, k = shape
    assert bipartite or N == M
    gen = torch.Generator().manual_seed(case_seed(shape, bipartite) if seed is None else seed)
    r = lambda *s: torch.randn(*s, generator=gen)                         # noqa: E731
    u = lambda *s: torch.rand(*s, generator=gen)                          # noqa: E731
    x = (r(B, C, N) * (u(1, C, 1) + 0.5) + (2 * u(1, C, 1) - 1)).contiguous()
    src = (r(B, C, M) * (u(1, C, 1) + 0.5) + (2 * u(1, C, 1) - 1)).contiguous() if bipartite else None
    return dict(shape=shape, x=x, src=src, idx=random_graph(B, N, M, k, gen), a=r(2 * C) * (1.5 / C ** 0.5),
                bias=torch.tensor([0.3]), eps=torch.tensor([0.3]), g=r(B, C, N) + 0.5)


def _grid(gen, *s):
    """Values on the 2^-2 grid in [-2, 2]."""
    return torch.randint(-8, 9, s, generator=gen).float() / 4.0


def make_exact_case(shape, bipartite, seed=None):
    """Operands on the 2^-2 grid in [-2, 2], eps = 0.25, a = 0, bias = 0.5.  Every fp32 operation of the GIN kernels is exact on
    them; so is every one of the GAT kernels when k is a power of two (p = 1 / k, sde = 0)."""
    B, C, N, M, k = shape
    assert bipartite or N == M
    gen = torch.Generator().manual_seed((case_seed(shape, bipartite) if seed is None else seed) + 7)
    return dict(shape=shape, x=_grid(gen, B, C, N), src=_grid(gen, B, C, M) if bipartite else None, idx=random_graph(B, N, M, k, gen),
                a=torch.zeros(2 * C), bias=torch.tensor([0.5]), eps=torch.tensor([0.25]), g=_grid(gen, B, C, N))


# (B, C, N, M, k) of the a = 0 family: in-degrees of at most a few hundred keep every partial sum within 24 bits
UNIFORM_SHAPES = [((2, 4, 257, 37, 2), True), ((2, 4, 257, 37, 4), True), ((2, 5, 70, 300, 8), True), ((2, 4, 257, 37, 16), True),
                  ((3, 3, 260, 260, 4), False), ((1, 2, 64, 64, 16), False)]
ONE_HOT_SHAPES = [((2, 4, 257, 37, 9), True), ((2, 3, 300, 300, 5), False), ((1, 2, 40, 700, 3), True)]


def make_one_hot_case(shape, bipartite, seed=None):
    """The key score decides alone: a[C] = 128 and nothing else, channel 0 of src a permutation of the integers 0 .. M - 1 per
    image, lists without repeats.  Two logits of a row differ by at least 128 > 104 = -ln(2^-150), so fp32 expf of every
    loser is 0 and p is exactly one-hot at the list's largest key; agg is the gather at that key, bit for bit (the fp64 softmax
    is NOT one-hot: its losers are e^-128 and more).  The other channels and g lie on the 2^-2 grid."""
    B, C, N, M, k = shape
    assert (bipartite or N == M) and k <= M
    gen = torch.Generator().manual_seed((case_seed(shape, bipartite) if seed is None else seed) + 13)
    s = _grid(gen, B, C, M)
    s[:, 0] = torch.rand(B, M, generator=gen).argsort(-1).float()
    a = torch.zeros(2 * C)
    a[C] = 128.0
    return dict(shape=shape, x=_grid(gen, B, C, N) if bipartite else s, src=s if bipartite else None,
                idx=distinct_graph(B, N, M, k, gen), a=a, bias=torch.tensor([0.5]), eps=torch.tensor([0.25]), g=_grid(gen, B, C, N))


def one_hot_expect(k):
    """(p, agg) of a one-hot case: 1 at the list's largest key (channel 0 of src IS the key's rank), the gather there."""
    s = _src(k["x"], k["src"])
    score = gather(s[:, :1], k["idx"]).squeeze(1)                                    # (B, N, k)
    best = score.argmax(-1, keepdim=True)
    p = torch.zeros_like(score).scatter_(-1, best, 1.0)
    return p, gather(s, k["idx"]).gather(-1, best.unsqueeze(1).expand(-1, s.shape[1], -1, -1)).squeeze(-1)
