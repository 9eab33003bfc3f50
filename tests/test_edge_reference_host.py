"""tests/edge_ref.py — the fp64 reference the GPU tests hold csrc/gkg_edge.hip to — pinned on the CPU, in double.

AGAINST AUTOGRAD.  The literal form of the reference (gather x_j, form x_j - x_i, 1x1 projection + bias, F.batch_norm in training
or eval mode or no norm, activation, max over k; for qc None the same on x_j alone: GraphSAGE's nn1) is differentiated by torch.
edge_ref's stats -> (mean0, invstd, a, c) -> fwd -> bwd_stats -> bwd, composed exactly the way gkgnet_amd.ops._EdgeAggregate composes
the four kernels, must give the same out, dQ, dQc, dgamma, dbeta and dbias to 1e-11.  The neighbour lists of this part hold no key
twice, so torch's own rule for exact ties does not enter; the two out-of-range entries stay.

SENSITIVITY.  For nine wrong formulas (no clamp, last maximum, a dropped mg / mgz term, ...) the wrong result is put through the
very report functions and bound constants the GPU tests use (edge_ref.fwd_report / bwd_report / SUM_TOL), on the GPU tests' own
inputs: each must land above the bound, or the bound could not tell it from the right formula."""
import math

import pytest
import torch
import torch.nn.functional as F

import edge_ref as E

EPS, MOM = 1e-5, 0.1


def _close(a, b, tol=1e-11):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _distinct_graph(B, N, M, k, gen):
    """Rows without a repeated key (k <= M), plus the two out-of-range entries, placed where they clamp onto no other entry."""
    idx = torch.rand(B, N, M, generator=gen).argsort(-1)[..., :k].contiguous()
    for row, slot, key, bad in ((idx[0, 0], 0, 0, -5), (idx[-1, -1], k - 1, M - 1, M + 7)):
        p = (row == key).nonzero()
        if p.numel():
            row[int(p[0])] = row[slot]
        row[slot] = bad
    return idx


def _post(y, norm, gamma, beta, rm, rv, code):
    if norm == "train" and y.numel() == y.shape[1]:
        # torch refuses a one-sample training batch: the written formula (mean = y, variance 0), differentiated all the same
        mean = y.mean(dim=(0, 2, 3), keepdim=True)
        var = ((y - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        y = (y - mean) / torch.sqrt(var + EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    elif norm is not None:
        y = F.batch_norm(y, rm, rv, gamma, beta, norm == "train", MOM, EPS)
    y = F.gelu(y) if code == 1 else (torch.relu(y) if code == 2 else y)
    return y.max(dim=-1).values


@pytest.mark.parametrize("with_qc", [True, False])
@pytest.mark.parametrize("code", [0, 1, 2])
@pytest.mark.parametrize("norm", ["train", "eval", None])
@pytest.mark.parametrize("shape", E.SHAPES)
def test_reference_matches_autograd_of_the_literal_form(shape, norm, code, with_qc):
    B, O, N, M, k = shape
    C = O + 2
    gen = torch.Generator().manual_seed(sum(shape) + 7 * code + (norm is not None) + with_qc)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)            # noqa: E731
    self_graph = with_qc and shape == E.SELF_GRAPH
    x = (r(B, C, N) + 1.0).requires_grad_(True)
    src = x if self_graph else (r(B, C, M) - 0.5).requires_grad_(True)
    W, bias = (r(O, C) / math.sqrt(C)).requires_grad_(True), r(O).requires_grad_(True)
    gamma = (torch.rand(O, generator=gen, dtype=torch.float64) + 0.5) * torch.where(torch.arange(O) % 4 == 1, -1.0, 1.0)
    gamma, beta = gamma.requires_grad_(True), r(O).requires_grad_(True)
    rm0, rv0 = r(O), torch.rand(O, generator=gen, dtype=torch.float64) + 0.5
    idx = _distinct_graph(B, N, M, k, gen)
    g = r(B, O, N)
    cnt = B * N * k

    # ---- the literal form, differentiated by torch
    x_j = E.gather(src, idx)                                                       # (B, C, N, k), clamped like the kernels
    d = x_j - x.unsqueeze(-1) if with_qc else x_j
    y = torch.einsum("oc,bcnk->bonk", W, d) + bias.view(1, -1, 1, 1)
    rm, rv = rm0.clone(), rv0.clone()
    want = _post(y, norm, gamma, beta, rm, rv, code)
    want.backward(g)

    # ---- the same function composed from edge_ref the way ops._EdgeAggregate composes the kernels
    with torch.no_grad():
        qs = torch.einsum("oc,bcm->bom", W, src)
        qc = torch.einsum("oc,bcn->bon", W, x) if with_qc else None
        zz = E.z(qs, qc, idx)
        mean0 = invstd = mg = mgz = dgamma = dbeta = None
        if norm == "train":
            sums, _ = E.stats(zz)
            mean0 = sums[:O] / cnt
            var = (sums[O:] / cnt - mean0 * mean0).clamp_min(0.0)
            invstd = torch.rsqrt(var + EPS)
            a = gamma * invstd
            c = beta - a * mean0
            if cnt > 1:
                assert _close((1 - MOM) * rm0 + MOM * (mean0 + bias), rm), "running_mean"
                assert _close((1 - MOM) * rv0 + MOM * var * (cnt / (cnt - 1)), rv), "running_var"
        elif norm == "eval":
            invstd = torch.rsqrt(rv0 + EPS)
            mean0 = rm0 - bias
            a = gamma * invstd
            c = beta - a * mean0
        else:
            a, c = torch.ones(O, dtype=torch.float64), bias.detach().clone()
        out, _, arg = E.fwd(zz, a, c, code)
        if norm is not None:
            sums, _ = E.bwd_stats(g, zz, arg, a, c, mean0, invstd, code)
            dbeta, dgamma = sums[:O], sums[O:]
            if norm == "train":
                mg, mgz = sums[:O] / cnt, sums[O:] / cnt
        dqs, dqc = E.bwd(g, zz, idx, M, arg, a, c, code, mean0, invstd, mg, mgz)
        if norm == "train":
            dbias = torch.zeros(O, dtype=torch.float64)
        elif norm == "eval":
            dbias = a * dbeta
        else:
            dbias = -dqc.sum(dim=(0, 2))
        # chain rule through the two per-node projections (C > O: W^T is injective, so this pins dQ and dQc themselves)
        dsrc = torch.einsum("oc,bom->bcm", W, dqs)
        dx = torch.einsum("oc,bon->bcn", W, dqc) if with_qc else None
        dW = torch.einsum("bom,bcm->oc", dqs, src)
        if with_qc:
            dW = dW + torch.einsum("bon,bcn->oc", dqc, x)
            if self_graph:
                dsrc, dx = dsrc + dx, None
    assert _close(out, want.detach()), "out"
    if self_graph:
        assert _close(dsrc, x.grad), "dx (self graph: dQ and dQc through the same projection)"
    else:
        assert _close(dsrc, src.grad), "dQ"
        if with_qc:
            assert _close(dx, x.grad), "dQc"
    assert _close(dW, W.grad), "dW"
    assert _close(dbias, bias.grad), "dbias"
    if norm is not None:
        assert _close(dgamma, gamma.grad), "dgamma"
        assert _close(dbeta, beta.grad), "dbeta"


def test_projected_gradients_pin_dq_and_dqc_directly():
    """Q and Qc as the leaves: z = Q[j] - Qc + bias -> train-mode BN -> GELU -> max.  dQ and dQc themselves, not W^T of them."""
    B, O, N, M, k = 2, 5, 33, 11, 4
    gen = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)            # noqa: E731
    qs, qc = r(B, O, M).requires_grad_(True), r(B, O, N).requires_grad_(True)
    gamma, beta = (r(O) + 0.2).requires_grad_(True), r(O).requires_grad_(True)
    idx = _distinct_graph(B, N, M, k, gen)
    g = r(B, O, N)
    want = _post(E.z(qs, qc, idx), "train", gamma, beta, None, None, 1)
    want.backward(g)
    with torch.no_grad():
        zz, cnt = E.z(qs, qc, idx), B * N * k
        sums, _ = E.stats(zz)
        mean0 = sums[:O] / cnt
        invstd = torch.rsqrt(sums[O:] / cnt - mean0 * mean0 + EPS)
        a = gamma * invstd
        c = beta - a * mean0
        out, _, arg = E.fwd(zz, a, c, 1)
        bs, _ = E.bwd_stats(g, zz, arg, a, c, mean0, invstd, 1)
        dqs, dqc = E.bwd(g, zz, idx, M, arg, a, c, 1, mean0, invstd, bs[:O] / cnt, bs[O:] / cnt)
    assert _close(out, want.detach()) and _close(dqs, qs.grad) and _close(dqc, qc.grad)
    assert _close(bs[O:], gamma.grad) and _close(bs[:O], beta.grad)


def test_first_maximum_and_nan_rules():
    v = torch.tensor([[1.0, 3.0, 3.0, 2.0], [0.0, 0.0, 0.0, 0.0], [1.0, float("nan"), float("nan"), 5.0],
                      [float("inf"), 2.0, float("inf"), 1.0]], dtype=torch.float64)
    mx, arg = E.first_max(v)
    assert arg.tolist() == [1, 0, 1, 0]
    assert mx[0] == 3 and mx[1] == 0 and math.isnan(float(mx[2])) and math.isinf(float(mx[3]))
    assert E.clamp(torch.tensor([-5, 0, 3, 4, 11]), 4).tolist() == [0, 0, 3, 3, 3]
    u = torch.tensor([-1.0, 0.0, 2.0], dtype=torch.float64)
    assert E.act(u, 2).tolist() == [0.0, 0.0, 2.0] and E.act_grad(u, 2).tolist() == [0.0, 0.0, 1.0]
    ug = u.clone().requires_grad_(True)
    F.gelu(ug).sum().backward()
    assert _close(E.act(u, 1), F.gelu(u)) and _close(E.act_grad(u, 1), ug.grad)


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def _gelu_tanh_grad(u):
    k0, k1 = math.sqrt(2.0 / math.pi), 0.044715
    t = torch.tanh(k0 * (u + k1 * u ** 3))
    return 0.5 * (1 + t) + 0.5 * u * (1 - t * t) * k0 * (1 + 3 * k1 * u * u)


def _wrap(idx, M):
    return idx % M                                                         # instead of the clamp


def _case64(shape, with_qc):
    k = E.make_case(shape, with_qc, E.case_seed(shape, with_qc))
    z32 = E.z(k["qs"], k["qc"], k["idx"])
    return k, z32


SENS_CASES = [(s, q) for s in E.SHAPES for q in (True, False)]


@pytest.mark.parametrize("shape,with_qc", SENS_CASES)
def test_each_wrong_formula_lands_above_the_bound_of_the_gpu_tests(shape, with_qc):
    B, O, N, M, kk = shape
    k, z32 = _case64(shape, with_qc)
    d = lambda t: t.double()                                              # noqa: E731
    idx, g, a, c, m0, inv, mg, mgz = (k[n] for n in ("idx", "g", "a", "c", "mean0", "invstd", "mg", "mgz"))
    z64 = d(z32)
    seen = []

    def above(name, err, bnd):
        seen.append(name)
        assert err > bnd, (name, shape, with_qc, err, bnd)

    # --- the right formula passes its own reports (the fp32 yardstick as the "kernel")
    for code in (0, 1, 2):
        out32, _, arg32 = E.fwd(z32, a, c, code)
        rep = E.fwd_report(out32, arg32, z32, a, c, code)
        assert rep["range"] and max(rep["out"], rep["pick"], rep["same"]) <= rep["bound"], rep

    # --- statistics (bound: SUM_TOL of the sum of |term|)
    ref_s, abs_s = E.stats(z64)
    wrap_idx = _wrap(idx, M)
    zw32 = E.z(k["qs"], k["qc"], wrap_idx)
    if M > 1 and not (wrap_idx == E.clamp(idx, M)).all():
        above("no clamp: stats", E.rel(E.stats(d(zw32))[0], ref_s, abs_s), E.SUM_TOL)
    if kk > 1:
        bn_only = torch.cat([z64[..., 0].sum(dim=(0, 2)), (z64[..., 0] ** 2).sum(dim=(0, 2))]) * kk
        above("statistics over (B, N) instead of (B, N, k)", E.rel(bn_only, ref_s, abs_s), E.SUM_TOL)

    for code in (0, 1, 2):
        _, _, arg = E.fwd(z64, d(a), d(c), code)
        arg = arg.to(torch.uint8)
        # --- backward statistics: exact-term acts are held to SUM_TOL, GELU to the fp32 bound; a wrong zhat is far above both
        ref_b, abs_b = E.bwd_stats(d(g), z64, arg, d(a), d(c), d(m0), d(inv), code)
        gp, zh, gm = E.bwd_terms(d(g), z64, arg, d(a), d(c), d(m0), d(inv), code)
        bad_b, _ = E.term_sums(gp, zh / d(inv).view(1, -1, 1), gm)
        y_b, _ = E.bwd_stats(g, z32, arg, a, c, m0, inv, code)
        above(f"zhat without invstd: bwd_stats act {code}", E.rel(bad_b, ref_b, abs_b), E.bound(E.rel(y_b, ref_b, abs_b)))

        # --- dense backward
        def rep_of(dqs, dqc, **kw):
            args = dict(mean0=m0, invstd=inv, mg=mg, mgz=mgz)
            args.update(kw)
            return E.bwd_report(dqs, dqc, g, z32, idx, M, arg, a, c, code, **args)

        ok_s, ok_c = E.bwd(d(g), z64, idx, M, arg, d(a), d(c), code, d(m0), d(inv), d(mg), d(mgz))
        rep = rep_of(ok_s, ok_c)
        assert rep["dqs"] == 0 and rep["dqc"] == 0

        A, M0, IV, MG, MGZ = (d(t).view(1, -1, 1, 1) for t in (a, m0, inv, mg, mgz))
        gp4 = _gp(g, z64, arg, a, c, code)
        if M > 1 and not (wrap_idx == E.clamp(idx, M)).all():
            bs, bc = E.bwd(d(g), d(zw32), wrap_idx, M, arg, d(a), d(c), code, d(m0), d(inv), d(mg), d(mgz))
            r2 = rep_of(bs, bc)
            above(f"no clamp: dqs act {code}", r2["dqs"], r2["bound_dqs"])
        wrong = {"mg term dropped": A * (gp4 - (z64 - M0) * IV * MGZ),
                 "mgz term dropped": A * (gp4 - MG),
                 "zhat without invstd": A * (gp4 - MG - (z64 - M0) * MGZ),
                 "winner-only gradient where the dense form is due": A * gp4}
        for name, dz in wrong.items():
            r2 = rep_of(*E.scatter(dz, idx, M))
            above(f"{name}: dqs act {code}", r2["dqs"], r2["bound_dqs"])
            above(f"{name}: dqc act {code}", r2["dqc"], r2["bound_dqc"])
        r2 = rep_of(ok_s, -ok_c)
        above(f"dqc sign flipped act {code}", r2["dqc"], r2["bound_dqc"])
        if code == 1:
            u = A * z64 + d(c).view(1, -1, 1, 1)
            win = torch.arange(kk).expand_as(z64) == arg.long().unsqueeze(-1)
            bs, bc = E.scatter(A * torch.where(win, d(g).unsqueeze(-1) * _gelu_tanh_grad(u), torch.zeros_like(u)), idx, M)
            r2 = E.bwd_report(bs, bc, g, z32, idx, M, arg, a, c, code)
            above("GELU derivative of the tanh approximation: dqs (winner-only)", r2["dqs"], r2["bound_dqs"])
            above("GELU derivative of the tanh approximation: dqc (winner-only)", r2["dqc"], r2["bound_dqc"])
    assert len(seen) >= 32, seen


def _gp(g, z64, arg, a, c, code):
    u = a.double().view(1, -1, 1, 1) * z64 + c.double().view(1, -1, 1, 1)
    win = torch.arange(z64.shape[-1]).expand_as(z64) == arg.long().unsqueeze(-1)
    return torch.where(win, g.double().unsqueeze(-1) * E.act_grad(u, code), torch.zeros_like(u))


@pytest.mark.parametrize("shape,with_qc", [(s, q) for s, q in SENS_CASES if s[4] > 1])
def test_last_maximum_differs_from_first_on_the_exact_inputs(shape, with_qc):
    """The tie rule shows only where ties are exact, and there the GPU test allows no mismatch at all: on its integer-valued
    inputs a last-maximum rule must name another k somewhere (and so must a wrapped index change ``out`` or ``argmax``)."""
    k = E.make_exact_case(shape, with_qc, E.case_seed(shape, with_qc))
    for code in (0, 2):
        z64 = E.z(k["qs"], k["qc"], k["idx"]).double()
        out, v, arg = E.fwd(z64, k["a"].double(), k["c"].double(), code)
        kk = shape[4]
        last = kk - 1 - E.first_max(v.flip(-1))[1]
        assert int((last != arg).sum()) > 0, ("last maximum", shape, code)
        outw, _, argw = E.fwd(E.z(k["qs"], k["qc"], k["idx"] % shape[3]).double(), k["a"].double(), k["c"].double(), code)
        sw, _ = E.stats(E.z(k["qs"], k["qc"], k["idx"] % shape[3]).double())
        assert not (torch.equal(outw, out) and torch.equal(argw, arg) and torch.equal(sw, E.stats(z64)[0])), ("no clamp", shape, code)
