"""tests/dense_ref.py — the fp64 reference the GPU tests hold csrc/gkg_dense.hip to — pinned on the CPU: its formulas (written
from the comments of include/gkg_hip.h) against torch autograd of F.batch_norm(training=True) followed by F.gelu, in double.
Output, dx, dgamma, dbeta and the running statistics; the SyncBN split (plain sums of two unequal row parts, added, with the total
count) must give the same; R == 1 is checked against the written formula only (torch refuses a one-row training batch).
Inputs are dense, contiguous (R, C) matrices: the CPU batch_norm backward problem tests/test_bn_memory_format.py records is about
channels-last strided gradients and is not touched here."""
import pytest
import torch
import torch.nn.functional as F

import dense_ref as D

EPS, MOM = 1e-5, 0.1


def _case(R, C, nb, seed, offset=3.0):
    g = torch.Generator().manual_seed(seed)
    std = torch.rand(nb, 1, C, generator=g, dtype=torch.float64) + 0.5
    y = torch.randn(nb, R, C, generator=g, dtype=torch.float64) * std + offset * std * torch.randn(nb, 1, C, generator=g, dtype=torch.float64)
    return dict(y=y, gamma=torch.rand(nb, C, generator=g, dtype=torch.float64) + 0.5, beta=torch.randn(nb, C, generator=g, dtype=torch.float64),
                bias=torch.randn(nb, C, generator=g, dtype=torch.float64), rm=torch.randn(nb, C, generator=g, dtype=torch.float64),
                rv=torch.rand(nb, C, generator=g, dtype=torch.float64) + 0.5, dout=torch.randn(nb, R, C, generator=g, dtype=torch.float64),
                res=torch.randn(nb, R, C, generator=g, dtype=torch.float64))


def _close(a, b, tol=1e-11):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("R,C,nb", [(2, 4, 1), (17, 8, 1), (64, 12, 4), (333, 36, 2)])
def test_reference_matches_autograd_of_batch_norm_and_gelu(R, C, nb, act):
    k = _case(R, C, nb, 100 * R + C + act)
    st = D.bn_stats(k["y"], k["gamma"], k["beta"], EPS)
    out, _ = D.affine_act(k["y"], st["a"], st["c"], act, res=k["res"])
    bw = D.bn_bwd(k["dout"], k["y"], st["a"], st["c"], st["mean"], st["invstd"], act)
    rm, rv = D.running_update(k["rm"], k["rv"], st["mean"], st["var"], k["bias"], R, MOM)
    for q in range(nb):
        # torch sees the conv output WITH its bias: it cancels in the output and in every gradient, and moves running_mean only
        x = (k["y"][q] + k["bias"][q]).clone().requires_grad_(True)
        gamma, beta = k["gamma"][q].clone().requires_grad_(True), k["beta"][q].clone().requires_grad_(True)
        trm, trv = k["rm"][q].clone(), k["rv"][q].clone()
        z = F.batch_norm(x, trm, trv, gamma, beta, True, MOM, EPS)
        o = (F.gelu(z) if act == 1 else z) + k["res"][q]
        o.backward(k["dout"][q])
        assert _close(out[q], o.detach()), "out"
        assert _close(bw["dy"][q], x.grad), "dx"
        assert _close(bw["sums"][q, 1], gamma.grad), "dgamma"
        assert _close(bw["sums"][q, 0], beta.grad), "dbeta"
        assert _close(rm[q], trm), "running_mean"
        assert _close(rv[q], trv), "running_var"
        assert _close(st["mean"][q] + k["bias"][q], x.detach().mean(0)) and _close(st["var"][q], x.detach().var(0, unbiased=False))


@pytest.mark.parametrize("act", [0, 1])
def test_row_scale_is_the_gradient_of_a_scaled_branch(act):
    """out = act(BN(y)) * row_scale[r // rows_per_scale]: autograd of exactly that against the reference's scaled backward."""
    R, C, rps = 45, 8, 7
    k = _case(R, C, 1, 5 + act)
    rs = torch.rand(-(-R // rps), dtype=torch.float64, generator=torch.Generator().manual_seed(1)) + 0.25
    st = D.bn_stats(k["y"], k["gamma"], k["beta"], EPS)
    out, _ = D.affine_act(k["y"], st["a"], st["c"], act, rs, rps, k["res"])
    bw = D.bn_bwd(k["dout"], k["y"], st["a"], st["c"], st["mean"], st["invstd"], act, rs, rps)
    x = k["y"][0].clone().requires_grad_(True)
    gamma, beta = k["gamma"][0].clone().requires_grad_(True), k["beta"][0].clone().requires_grad_(True)
    z = F.batch_norm(x, None, None, gamma, beta, True, MOM, EPS)
    o = (F.gelu(z) if act == 1 else z) * rs[torch.arange(R) // rps][:, None] + k["res"][0]
    o.backward(k["dout"][0])
    assert _close(out[0], o.detach()) and _close(bw["dy"][0], x.grad)
    assert _close(bw["sums"][0, 1], gamma.grad) and _close(bw["sums"][0, 0], beta.grad)


@pytest.mark.parametrize("act", [0, 1])
def test_syncbn_split_adds_up_to_the_whole_matrix(act):
    """Two unequal row parts: plain sums added, total count -> the statistics / gradients of the whole matrix."""
    R, C, nb, cut = 101, 12, 2, 37
    k = _case(R, C, nb, 9 + act)
    whole = D.bn_stats(k["y"], k["gamma"], k["beta"], EPS)
    parts = [slice(0, cut), slice(cut, R)]
    sums = sum(D.col_sums(k["y"][:, p]) for p in parts)
    st = D.bn_from_sums(sums, float(R), k["gamma"], k["beta"], EPS)
    for name in ("mean", "var", "invstd", "a", "c"):
        assert _close(st[name], whole[name], 1e-9), name
    want = D.bn_bwd(k["dout"], k["y"], whole["a"], whole["c"], whole["mean"], whole["invstd"], act)
    dz = [D.bn_bwd_dz(k["dout"][:, p], k["y"][:, p], st["a"], st["c"], act) for p in parts]
    local = [D.bn_bwd_sums(d, k["y"][:, p], st["mean"], st["invstd"])[0] for d, p in zip(dz, parts)]
    tot = local[0] + local[1]
    assert _close(tot, want["sums"], 1e-9)                                   # local dgamma / dbeta add up
    dy = torch.cat([D.bn_bwd_apply(d, k["y"][:, p], st["a"], st["mean"], st["invstd"], tot, float(R)) for d, p in zip(dz, parts)], 1)
    assert _close(dy, want["dy"], 1e-9)


def test_one_row_follows_the_written_formula():
    """R == 1: variance 0, invstd = 1 / sqrt(eps), the output is beta, the running variance takes the (guarded) biased estimate 0
    and every input gradient vanishes: dy = a * (dz - dz - yhat * ...) with yhat = 0."""
    k = _case(1, 8, 1, 77)
    st = D.bn_stats(k["y"], k["gamma"], k["beta"], EPS)
    assert torch.equal(st["mean"], k["y"][:, 0]) and torch.equal(st["var"], torch.zeros(1, 8, dtype=torch.float64))
    assert _close(st["invstd"], torch.full((1, 8), EPS ** -0.5, dtype=torch.float64))
    assert _close(st["a"], k["gamma"] * EPS ** -0.5)
    out, _ = D.affine_act(k["y"], st["a"], st["c"], 0)
    assert _close(out[:, 0], k["beta"], 1e-9)
    rm, rv = D.running_update(k["rm"], k["rv"], st["mean"], st["var"], k["bias"], 1, MOM)
    assert _close(rm, (1 - MOM) * k["rm"] + MOM * (k["y"][:, 0] + k["bias"])) and _close(rv, (1 - MOM) * k["rv"])
    bw = D.bn_bwd(k["dout"], k["y"], st["a"], st["c"], st["mean"], st["invstd"], 0)
    assert float(bw["dy"].abs().max()) == 0.0
    assert torch.equal(bw["sums"][:, 0], k["dout"][:, 0]) and float(bw["sums"][:, 1].abs().max()) == 0.0


def test_xm_column_map_and_layout_passes():
    assert D.xm_cols(8, 0).tolist() == list(range(8))
    assert D.xm_cols(8, 4).tolist() == [0, 1, 2, 3, 8, 9, 10, 11]             # chunks of 4 interleaved with the m half
    B, C, N = 2, 3, 5
    x = torch.arange(B * C * N, dtype=torch.float64).view(B, C, N)
    tm = D.nchw_to_tm(x)
    assert tm.shape == (B * N, C) and tm[N + 2, 1] == x[1, 1, 2]
    back, _ = D.tm_affine_to_nchw(tm, B, C, N)
    assert torch.equal(back, x)
    a, c = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), torch.tensor([0.5, 0.0, -1.0], dtype=torch.float64)
    sc = torch.tensor([2.0, 0.0], dtype=torch.float64)
    got, _ = D.tm_affine_to_nchw(tm, B, C, N, a, c, x, sc)
    assert torch.equal(got, (a[None, :, None] * x + c[None, :, None]) * sc[:, None, None] + x)
    o, o_tm, _ = D.tm_affine_to_nchw_dual(tm, B, C, N, a, c, tm)
    assert torch.equal(o_tm, a * tm + c + tm) and torch.equal(o, D.tm_affine_to_nchw(o_tm, B, C, N)[0])
    assert torch.equal(D.nchw_to_tm(x, sc, tm), (2 * tm).view(B, N, C).mul(sc[:, None, None]).view(B * N, C))
    p, _ = D.avgpool_tm(torch.arange(2 * 5 * 5 * 1, dtype=torch.float64), 2, 5, 5, 1, 2)
    want = F.avg_pool2d(torch.arange(50, dtype=torch.float64).view(2, 1, 5, 5), 2, 2)
    assert torch.equal(p.view(2, 2, 2), want.view(2, 2, 2))


@pytest.mark.parametrize("act", [0, 1])
def test_eval_mode_backward_matches_autograd(act):
    """Frozen BN (running statistics): dy, dgamma, dbeta and the gradient of the conv bias in front of it."""
    R, C = 37, 8
    k = _case(R, C, 1, 21 + act)
    inv = 1.0 / torch.sqrt(k["rv"] + EPS)
    a = k["gamma"] * inv
    c = k["beta"] + a * (k["bias"] - k["rm"])                      # gkg_bn_eval_affine
    x = k["y"][0].clone().requires_grad_(True)
    gamma, beta, bias = (k[n][0].clone().requires_grad_(True) for n in ("gamma", "beta", "bias"))
    z = F.batch_norm(x + bias, k["rm"][0], k["rv"][0], gamma, beta, False, MOM, EPS)
    (F.gelu(z) if act == 1 else z).backward(k["dout"][0])
    dz = D.bn_bwd_dz(k["dout"], k["y"], a, c, act)
    got, _ = D.bn_eval_bwd_params(dz, k["y"], a, k["rm"], k["rv"], k["bias"], EPS)
    assert _close(D.bn_eval_bwd(k["dout"], k["y"], a, c, act)[0], x.grad)
    assert _close(got["dgamma"][0], gamma.grad) and _close(got["dbeta"][0], beta.grad) and _close(got["dbias"][0], bias.grad)
