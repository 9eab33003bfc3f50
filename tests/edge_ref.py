"""Plain torch restatement of what include/gkg_hip.h promises for the gather kernels of EdgeConv and GraphSAGE (csrc/gkg_edge.hip,
the "EdgeConv aggregation" block of the header): gkg_edge_stats, gkg_edge_fwd, gkg_edge_bwd_stats, gkg_edge_bwd.

Every function computes in the dtype of its inputs.  Called with ``.double()`` operands it is the REFERENCE the GPU tests hold the
kernels to; called with the fp32 operands themselves it is the YARDSTICK: the error an honest fp32 implementation of the same
formula makes against the fp64 reference.  tests/test_edge_reference_host.py pins these formulas to torch autograd of the literal
form (gather, subtract, 1x1 projection, F.batch_norm, activation, max over k) in double on the CPU, and shows that the bounds below
tell each of a list of wrong formulas from the right one.

The kernels form z = Q[j] - Qc in fp32 before anything else, so the fp64 reference of a GPU test starts from that fp32 difference,
widened (``z(qs, qc, idx).double()`` with the fp32 operands): the rounding of the difference is one the contract allows.  Everything
after z takes ``z`` as an argument for that reason.

Shapes: qs (B, O, M), qc (B, O, N) or None (Qc = 0: GraphSAGE's nn1), idx (B, N, k) int64, z / v (B, O, N, k), per-channel
parameters (O,), g / out / argmax (B, O, N).  The module also holds what the GPU file and the host file must share so that they
cannot drift: the bound constants, the shape list and the input generators.  A helper module, not a test module and not a conftest."""
import math

import torch

# ------------------------------------------------------------------------------------------------------------------ the bar
# |got - ref| / scale <= max(K * yardstick error, FLOOR) (measured figures: EXPERIMENTS.md "EdgeConv gather kernels vs fp64").
#   K      covers erff / __expf against torch's erf / exp and the fma contraction the kernels use.
#   FLOOR  2 fp32 ulp of the scale (2^-22): the store of the result is one rounding of a value no larger than its scale (2^-24),
#          GELU and its derivative add a handful more (the erf argument, erf, 1 + erf, two products), and a yardstick that happens
#          to round exactly on a small case must not turn the bound into zero.
#   SUM_TOL  the fp64-accumulated statistics: their terms are exact, only the order of the fp64 additions differs.
K = 4.0
FLOOR = 2.0 ** -22
SUM_TOL = 1e-12

# (B, O, N, M, k): see tests/test_hip_edge_fp64.py for what each one is there for
SHAPES = [(1, 1, 1, 1, 1), (2, 5, 255, 37, 9), (2, 5, 256, 37, 9), (2, 5, 257, 37, 9), (3, 8, 513, 513, 3), (1, 20, 300, 5, 4),
          (2, 12, 64, 600, 255), (4, 3, 70, 1000, 6)]
SELF_GRAPH = (3, 8, 513, 513, 3)          # qs and qc are the same buffer there, as EdgeConv2d passes them without a source


# ------------------------------------------------------------------------------------------------------------------ gather
def clamp(idx, M):
    """Out-of-range neighbour indices are clamped into [0, M - 1]."""
    return idx.clamp(0, M - 1)


def _flat(idx, B, O, M):
    """Flat positions of the clamped (B, N, k) indices in a (B, O, M) tensor, shaped (B, O, N * k)."""
    N, k = idx.shape[1:]
    row = (torch.arange(B, device=idx.device).view(B, 1, 1) * O + torch.arange(O, device=idx.device).view(1, O, 1)) * M
    return row + clamp(idx, M).reshape(B, 1, N * k)


def gather(q, idx):
    """q (B, O, M) at the clamped idx (B, N, k) -> (B, O, N, k)."""
    B, O, M = q.shape
    N, k = idx.shape[1:]
    return q.reshape(-1)[_flat(idx, B, O, M)].reshape(B, O, N, k)


def z(qs, qc, idx):
    """Q[j] - Qc, or Q[j] when qc is None; (B, O, N, k) in the dtype of qs."""
    zj = gather(qs, idx)
    return zj if qc is None else zj - qc.unsqueeze(-1)


def _ch(p):
    return p.view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------ activation
def act(u, code):
    """0 none, 1 GELU (erf form), 2 ReLU."""
    if code == 1:
        return u * 0.5 * (1.0 + torch.erf(u * (1.0 / math.sqrt(2.0))))
    if code == 2:
        return torch.relu(u)                                               # NaN stays NaN, as in the literal form
    return u


def act_grad(u, code):
    """Derivative of ``act``; ReLU: 0 at u <= 0."""
    if code == 1:
        return 0.5 * (1.0 + torch.erf(u * (1.0 / math.sqrt(2.0)))) + u * torch.exp(-0.5 * u * u) * (1.0 / math.sqrt(2.0 * math.pi))
    if code == 2:
        return torch.where(u > 0, torch.ones_like(u), torch.zeros_like(u))
    return torch.ones_like(u)


def act_grad_mag(u, code):
    """The magnitude of act_grad's intermediates: what an error of it is measured against.  GELU' = 0.5 (1 + erf) + u pdf(u)
    vanishes at u = -0.7518 and decays like exp(-u^2 / 2) below it while 1 and erf stay of size 1, so a relative error of the
    RESULT has no bound in any precision; 0.5 (1 + |erf|) + |u| pdf(u) is what the roundings of its terms scale with."""
    if code == 1:
        return 0.5 * (1.0 + torch.erf(u * (1.0 / math.sqrt(2.0))).abs()) + u.abs() * torch.exp(-0.5 * u * u) * (1.0 / math.sqrt(2.0 * math.pi))
    return act_grad(u, code)


# ------------------------------------------------------------------------------------------------------------------ forward
def stats(zz):
    """gkg_edge_stats: (2 O) sums of z and z^2 over all (b, n, k); and the sums of |term| (their scale; z^2 is its own)."""
    s1, s2 = zz.sum(dim=(0, 2, 3)), (zz * zz).sum(dim=(0, 2, 3))
    return torch.cat([s1, s2]), torch.cat([zz.abs().sum(dim=(0, 2, 3)), s2])


def first_max(v):
    """(max over the last dim, the first k attaining it).  NaN propagates: the first NaN wins."""
    k = v.shape[-1]
    mx = v.max(dim=-1).values
    hit = (v == mx.unsqueeze(-1)) | (torch.isnan(v) & torch.isnan(mx).unsqueeze(-1))
    ar = torch.arange(k, device=v.device).expand_as(v)
    return mx, torch.where(hit, ar, torch.full_like(ar, k)).min(dim=-1).values


def fwd(zz, a, c, code):
    """gkg_edge_fwd: out = max_k act(a z + c) -> (out (B, O, N), the per-edge values v (B, O, N, k), the first maximising k)."""
    v = act(_ch(a) * zz + _ch(c), code)
    out, arg = first_max(v)
    return out, v, arg


def fwd_mag(zz, a, c):
    """|a z| + |c| per edge: the scale a forward error is measured against."""
    return (_ch(a) * zz).abs() + _ch(c).abs()


def at(v, arg):
    """v (B, O, N, k) at arg (B, O, N) -> (B, O, N)."""
    return v.gather(-1, arg.long().unsqueeze(-1)).squeeze(-1)


# ------------------------------------------------------------------------------------------------------------------ backward
def bwd_terms(g, zz, argmax, a, c, mean0, invstd, code):
    """At the argmax elements: g' = g act'(a z + c), zhat = (z - mean0) invstd and the scale of g' (|g| act_grad_mag), (B, O, N)."""
    zw = at(zz, argmax)
    u = a.view(1, -1, 1) * zw + c.view(1, -1, 1)
    return g * act_grad(u, code), (zw - mean0.view(1, -1, 1)) * invstd.view(1, -1, 1), g.abs() * act_grad_mag(u, code)


def term_sums(gp, zhat, gp_mag):
    """[sum g', sum g' zhat] per channel, (2 O); and the sums of the terms' scales."""
    return (torch.cat([gp.sum(dim=(0, 2)), (gp * zhat).sum(dim=(0, 2))]),
            torch.cat([gp_mag.sum(dim=(0, 2)), (gp_mag * zhat.abs()).sum(dim=(0, 2))]))


def bwd_stats(g, zz, argmax, a, c, mean0, invstd, code):
    """gkg_edge_bwd_stats: dbeta, dgamma and (divided by B N k) the two means of the BN backward.  ``argmax`` is an input."""
    return term_sums(*bwd_terms(g, zz, argmax, a, c, mean0, invstd, code))


def _dz(g, zz, argmax, a, c, code, mean0, invstd, mg, mgz, mag):
    k = zz.shape[-1]
    win = torch.arange(k, device=zz.device).expand_as(zz) == argmax.long().unsqueeze(-1)
    u = _ch(a) * zz + _ch(c)
    gp = torch.where(win, g.unsqueeze(-1) * (act_grad_mag(u, code) if mag else act_grad(u, code)), torch.zeros_like(zz))
    if mg is None:
        return _ch(a).abs() * gp.abs() if mag else _ch(a) * gp
    zhat = (zz - _ch(mean0)) * _ch(invstd)
    if mag:
        return _ch(a).abs() * (gp.abs() + _ch(mg).abs() + (zhat * _ch(mgz)).abs())
    return _ch(a) * (gp - _ch(mg) - zhat * _ch(mgz))


def scatter(dz, idx, M):
    """Per-edge dz (B, O, N, k) -> (dqs = the index_add_ over the clamped indices, dqc = -sum_k dz)."""
    B, O, N, k = dz.shape
    dqs = torch.zeros(B * O * M, dtype=dz.dtype, device=dz.device)
    dqs.index_add_(0, _flat(idx, B, O, M).reshape(-1), dz.reshape(-1))
    # both sums run left to right in the dtype of dz: "plain fp32" for the yardstick means one accumulator (torch.sum's cascade
    # summation is more accurate than that, and would hold a k = 255 loop to a bar no accumulate loop meets)
    acc = torch.zeros(B, O, N, dtype=dz.dtype, device=dz.device)
    for kk in range(k):
        acc = acc + dz[..., kk]
    return dqs.view(B, O, M), -acc


def bwd(g, zz, idx, M, argmax, a, c, code, mean0=None, invstd=None, mg=None, mgz=None):
    """gkg_edge_bwd -> (dqs (B, O, M), dqc (B, O, N)).  With mg / mgz the dense form dz = a (g' [k == argmax] - mg - zhat mgz) on
    every edge; with mg None only the winning edge carries gradient.  dqs[clamped idx] += dz, dqc = -sum_k dz."""
    return scatter(_dz(g, zz, argmax, a, c, code, mean0, invstd, mg, mgz, False), idx, M)


def bwd_mag(g, zz, idx, M, argmax, a, c, code, mean0=None, invstd=None, mg=None, mgz=None):
    """The same scatter applied to |dz| taken term by term, |a| (|g| act_grad_mag + |mg| + |zhat mgz|): the scale the backward
    error is measured against."""
    s, n = scatter(_dz(g, zz, argmax, a, c, code, mean0, invstd, mg, mgz, True), idx, M)
    return s, -n


# ------------------------------------------------------------------------------------------------------------------ error measure
def rel(got, ref, scale):
    """max |got - ref| / scale, in double (0 where both scale and difference vanish)."""
    d = (got.double() - ref.double()).abs()
    return float((d / scale.double().clamp_min(1e-300)).max()) if d.numel() else 0.0


def bound(yard_err):
    return max(K * yard_err, FLOOR)


# ------------------------------------------------------------------------------------------------------------------ reports
def fwd_report(out, arg, z32, a, c, code):
    """A forward result (out fp32, arg integer, both (B, O, N), CPU) against the fp64 reference of the fp32 operands.
      out   |out - fp64 maximum|
      pick  |fp64 value at the result's argmax - fp64 maximum|        (no exclusions: near-ties pass by their value)
      same  |out - the fp32 yardstick's value of that same edge|
    each divided by |a z| + |c| of the edges involved; ``yard`` is the yardstick's own ``out`` error, ``bound`` what all three
    must stay under.  ``range`` says every argmax is in [0, k)."""
    k = z32.shape[-1]
    z64, a64, c64 = z32.double(), a.double(), c.double()
    out64, v64, arg64 = fwd(z64, a64, c64, code)
    out32, v32, arg32 = fwd(z32, a, c, code)
    mag = fwd_mag(z64, a64, c64)
    in_range = bool(((arg >= 0) & (arg < k)).all())
    ag = arg.long().clamp(0, k - 1)
    m_ref, m_got = at(mag, arg64), at(mag, ag)
    yard = rel(out32, out64, torch.maximum(m_ref, at(mag, arg32)))
    both = torch.maximum(m_ref, m_got)
    return dict(range=in_range, out=rel(out, out64, both), pick=rel(at(v64, ag), out64, both), same=rel(out, at(v32, ag), m_got),
                yard=yard, bound=bound(yard))


def bwd_report(dqs, dqc, g, z32, idx, M, arg, a, c, code, mean0=None, invstd=None, mg=None, mgz=None):
    """A backward result (fp32, CPU; dqc may be None) against the fp64 reference, relative to bwd_mag; the yardstick is the fp32
    evaluation of the same formula (index_add_ in fp32).  -> dict(dqs, dqc, yard_dqs, yard_dqc, bound_dqs, bound_dqc)."""
    d = lambda t: None if t is None else t.double()                       # noqa: E731
    r_s, r_c = bwd(d(g), d(z32), idx, M, arg, d(a), d(c), code, d(mean0), d(invstd), d(mg), d(mgz))
    m_s, m_c = bwd_mag(d(g), d(z32), idx, M, arg, d(a), d(c), code, d(mean0), d(invstd), d(mg), d(mgz))
    y_s, y_c = bwd(g, z32, idx, M, arg, a, c, code, mean0, invstd, mg, mgz)
    ys, yc = rel(y_s, r_s, m_s), rel(y_c, r_c, m_c)
    return dict(dqs=rel(dqs, r_s, m_s), dqc=None if dqc is None else rel(dqc, r_c, m_c), yard_dqs=ys, yard_dqc=yc,
                bound_dqs=bound(ys), bound_dqc=bound(yc))


# ------------------------------------------------------------------------------------------------------------------ inputs
def random_graph(B, N, M, k, gen):
    """randint lists (repeats are natural), every third row repeating its first neighbour, two out-of-range entries."""
    idx = torch.randint(0, M, (B, N, k), generator=gen)
    if k >= 2:
        idx[:, ::3, 1] = idx[:, ::3, 0]
    idx[0, 0, 0], idx[-1, -1, -1] = -5, M + 7
    return idx


def case_seed(shape, with_qc):
    """The seed both test files use for ``shape``.  The base is one at which the single element of (1, 1, 1, 1, 1) has
    a z + c > 0 with and without qc: a dead ReLU there has no gradient for a wrong formula to get wrong."""
    return 1003 + sum(shape) + int(with_qc)


def make_case(shape, with_qc, seed):
    """fp32 CPU operands of one problem.  Q and Qc carry per-channel offsets of up to three standard deviations (so z is not
    centred and the statistics see cancellation), a is negative on every fourth channel (from the second), |a| in [0.5, 1.5],
    c ~ N(0, 1); mean0 sits near the mean of z, invstd in [0.5, 1.5]; mg, mgz ~ 0.1 N(0, 1); g ~ N(0.5, 1)."""
    B, O, N, M, k = shape
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                         # noqa: E731
    u = lambda *s: torch.rand(*s, generator=gen)                          # noqa: E731
    std = u(1, O, 1) + 0.5
    off_s, off_c = (6 * u(1, O, 1) - 3) * std, (6 * u(1, O, 1) - 3) * std
    qs = (r(B, O, M) * std + off_s).contiguous()
    if not with_qc:
        qc, off_c = None, torch.zeros(1, O, 1)
    elif shape == SELF_GRAPH:
        qc, off_c = qs, off_s
    else:
        qc = (r(B, O, N) * std + off_c).contiguous()
    sign = torch.ones(O)
    sign[1::4] = -1.0
    return dict(shape=shape, qs=qs, qc=qc, idx=random_graph(B, N, M, k, gen), a=(u(O) + 0.5) * sign, c=r(O),
                mean0=((off_s - off_c).reshape(O) + 0.1 * r(O)).contiguous(), invstd=u(O) + 0.5, mg=0.1 * r(O), mgz=0.1 * r(O),
                g=r(B, O, N) + 0.5, arg_rand=torch.randint(0, k, (B, O, N), generator=gen).to(torch.uint8))


def make_exact_case(shape, with_qc, seed):
    """Operands on which every fp32 operation of the kernels is exact: integer Q, Qc in [-8, 8], a in {+-0.5, +-1, +-2}, integer c
    in [-4, 4], g on a 2^-4 grid.  Full of exact ties (repeated neighbours, ReLU zeros, equal integers)."""
    B, O, N, M, k = shape
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()     # noqa: E731
    qs = ri(-8, 8, B, O, M)
    qc = None if not with_qc else (qs if shape == SELF_GRAPH else ri(-8, 8, B, O, N))
    a = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (O,), generator=gen)] * (2 * torch.randint(0, 2, (O,), generator=gen) - 1)
    return dict(shape=shape, qs=qs, qc=qc, idx=random_graph(B, N, M, k, gen), a=a.float(), c=ri(-4, 4, O), g=ri(-32, 32, B, O, N) / 16.0)
