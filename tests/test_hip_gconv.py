"""GraphSAGE / GIN / graph-attention aggregations of GraphConv2d on the GPU (csrc/gkg_gconv.hip; SAGE on csrc/gkg_edge.hip
with qc = NULL): the HIP path against the literal reference form on the same device, the operators against an fp64 torch
composition, the reference fixtures F18-F21, bit-identical backward runs, the memory the HIP path saves, the
unchanged edge path, and (against the literal module in double) GIN / GAT beyond one workgroup, B = 1, non-contiguous inputs, partial
gradient requests and a captured hipGraph.  The kernels themselves are held to fp64 through the C ABI in tests/test_hip_gconv_fp64.py."""
import copy

import numpy as np
import pytest
import torch

from test_gconv_host import GRAPHER_CASES, LABEL_CASES, make_grapher, make_label
from util import check_indices, grads_from, load_fixture, state_from

pytestmark = pytest.mark.gpu
TOL = dict(atol=1e-3, rtol=1e-3)


def _t(a):
    return torch.from_numpy(np.array(a)).cuda()


def _literal(mod):
    """The same module with the HIP plan switched off: every call takes the literal reference form."""
    mod._hip_plan = lambda x: None
    return mod


def _edge(idx):
    B, N, k = idx.shape
    return torch.stack([idx, torch.arange(N, device=idx.device).view(1, N, 1).expand(B, N, k)])


def _make(conv, C, out, act, norm):
    from gkgnet_amd.graph import GINConv2d, GraphAtten, GraphSAGE
    mod = {"sage": GraphSAGE, "gin": GINConv2d, "gat": GraphAtten}[conv](C, out, act, norm, True).cuda()
    with torch.no_grad():
        for p in mod.parameters():
            p.add_(0.1 * torch.randn_like(p))
        for m in mod.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5)
        if conv == "gin":
            mod.eps.fill_(0.3)
    return mod


@pytest.fixture
def local_bn():
    from gkgnet_amd import layers
    old = dict(layers.norm_cfg)
    layers.norm_cfg.update(type="BN")
    yield
    layers.norm_cfg.clear(); layers.norm_cfg.update(old)


@pytest.mark.parametrize("conv", ["sage", "gin", "gat"])
@pytest.mark.parametrize("bipartite", [False, True])
@pytest.mark.parametrize("norm,act,train", [("batch", "gelu", True), ("batch", "relu", True), ("batch", "gelu", False),
                                            (None, "relu", True), (None, "gelu", True)])
def test_module_hip_matches_literal_form(conv, norm, act, train, bipartite, local_bn):
    torch.manual_seed(7)
    B, C, N, M, k, out = 3, 24, 50, 37, 6, 40
    mod = _make(conv, C, out, act, norm)
    ref = _literal(copy.deepcopy(mod))
    mod.train(train); ref.train(train)
    x = torch.randn(B, C, N, 1, device="cuda", requires_grad=True)
    y = torch.randn(B, C, M, 1, device="cuda", requires_grad=True) if bipartite else None
    assert mod._hip_plan(x) is not None
    Mk = M if bipartite else N
    idx = torch.stack([torch.randperm(Mk, device="cuda")[:k] for _ in range(B * N)]).view(B, N, k)
    edge = _edge(idx)
    outp = mod(x, edge, y)
    x2 = x.detach().clone().requires_grad_(True)
    y2 = None if y is None else y.detach().clone().requires_grad_(True)
    want = ref(x2, edge, y2)
    assert outp.shape == want.shape
    assert torch.allclose(outp, want, atol=2e-5, rtol=1e-5), float((outp - want).abs().max())
    g = torch.randn_like(want)
    outp.backward(g); want.backward(g)
    assert torch.allclose(x.grad, x2.grad, atol=5e-5, rtol=1e-4), float((x.grad - x2.grad).abs().max())
    if bipartite:
        assert torch.allclose(y.grad, y2.grad, atol=5e-5, rtol=1e-4), float((y.grad - y2.grad).abs().max())
    for (name, p), (_, q) in zip(mod.named_parameters(), ref.named_parameters()):
        gp = torch.zeros_like(p) if p.grad is None else p.grad
        gq = torch.zeros_like(q) if q.grad is None else q.grad
        # a.bias and the a[:C] half of a.weight: their exact gradient is 0 (softmax is shift-invariant) -> rounding noise
        assert torch.allclose(gp, gq, atol=2e-4, rtol=1e-4), (name, float((gp - gq).abs().max()))
    for m, r in zip(mod.modules(), ref.modules()):
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            assert torch.allclose(m.running_mean, r.running_mean, atol=1e-5)
            assert torch.allclose(m.running_var, r.running_var, atol=1e-5, rtol=1e-5)
            assert int(m.num_batches_tracked) == int(r.num_batches_tracked)


@pytest.mark.parametrize("k,hip", [(255, True), (256, False)])
def test_sage_k_boundary_of_the_hip_path(k, hip, local_bn, monkeypatch):
    """The edge kernels' uint8 argmax holds k <= 255: GraphSAGE runs them up to there and the literal form above.  No norm here:
    the maximum over 255 of 300 keys is nearly the same number for every node, and a BatchNorm behind it (nn2) divides by the
    standard deviation of that: both fp32 paths then sit 1.5e-4 from the literal form in double (measured), which says nothing
    about either.  The train-mode statistics at k = 255 are held to fp64 in tests/test_hip_edge_fp64.py."""
    from gkgnet_amd import ops
    torch.manual_seed(7)
    B, C, N, out = 1, 8, 300, 16
    mod = _make("sage", C, out, "gelu", None)
    ref = _literal(copy.deepcopy(mod))
    x = torch.randn(B, C, N, 1, device="cuda", requires_grad=True)
    assert mod._hip_plan(x) is not None
    edge = _edge(torch.randint(0, N, (B, N, k), device="cuda"))
    real, spy = ops.edge_aggregate, []
    monkeypatch.setattr(ops, "edge_aggregate", lambda *a, **kw: (spy.append(k), real(*a, **kw))[1])
    outp = mod(x, edge)
    monkeypatch.setattr(ops, "edge_aggregate", real)
    assert spy == ([k] if hip else []), spy
    x2 = x.detach().clone().requires_grad_(True)
    want = ref(x2, edge)
    assert outp.shape == want.shape
    assert torch.allclose(outp, want, atol=2e-5, rtol=1e-5), float((outp - want).abs().max())
    g = torch.randn_like(want)
    outp.backward(g); want.backward(g)
    assert torch.allclose(x.grad, x2.grad, atol=5e-5, rtol=1e-4), float((x.grad - x2.grad).abs().max())
    for (name, p), (_, q) in zip(mod.named_parameters(), ref.named_parameters()):
        gp = torch.zeros_like(p) if p.grad is None else p.grad
        gq = torch.zeros_like(q) if q.grad is None else q.grad
        assert torch.allclose(gp, gq, atol=2e-4, rtol=1e-4), (name, float((gp - gq).abs().max()))


# ------------------------------------------------------------------------------------------- operators vs fp64 torch
def _random_graph(B, N, M, k, gen):
    idx = torch.randint(0, M, (B, N, k), generator=gen)
    idx[:, ::3, 1] = idx[:, ::3, 0]                     # rows that repeat a neighbour
    idx[0, 0, 0], idx[-1, -1, -1] = -5, M + 7          # out of range: clamped into [0, M)
    return idx


def _gather64(src, idx):
    B, C, M = src.shape
    N, k = idx.shape[1:]
    j = idx.clamp(0, M - 1)
    return torch.gather(src, 2, j.reshape(B, 1, N * k).expand(B, C, N * k)).reshape(B, C, N, k)


@pytest.mark.parametrize("B,C,N,M,k,bip", [(2, 8, 17, 17, 3, False), (3, 20, 40, 11, 5, True), (1, 64, 100, 100, 9, False),
                                           (4, 12, 9, 300, 16, True)])
def test_gin_op_matches_fp64(B, C, N, M, k, bip):
    from gkgnet_amd import ops
    gen = torch.Generator().manual_seed(B * 1000 + N)
    x = torch.randn(B, C, N, generator=gen)
    y = torch.randn(B, C, M, generator=gen) if bip else None
    idx = _random_graph(B, N, M if bip else N, k, gen)
    eps = torch.tensor([0.25])
    g = torch.randn(B, C, N, generator=gen)
    xd, ed = x.double().requires_grad_(True), eps.double().requires_grad_(True)
    yd = None if y is None else y.double().requires_grad_(True)
    want = (1 + ed) * xd + _gather64(xd if yd is None else yd, idx).sum(-1)
    want.backward(g.double())
    xc, ec = x.cuda().requires_grad_(True), eps.cuda().requires_grad_(True)
    yc = None if y is None else y.cuda().requires_grad_(True)
    got = ops.gin_aggregate(xc, idx.cuda(), ec, yc)
    got.backward(g.cuda())
    assert torch.allclose(got.double().cpu(), want, atol=1e-5, rtol=1e-5)
    assert torch.allclose(xc.grad.double().cpu(), xd.grad, atol=1e-5, rtol=1e-5)
    if bip:
        assert torch.allclose(yc.grad.double().cpu(), yd.grad, atol=1e-5, rtol=1e-5)
    assert torch.allclose(ec.grad.double().cpu(), ed.grad, atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("B,C,N,M,k,bip,bias", [(2, 8, 17, 17, 3, False, True), (3, 20, 40, 11, 5, True, True),
                                                (1, 64, 100, 100, 9, False, False), (4, 12, 9, 300, 16, True, True)])
def test_gat_op_matches_fp64(B, C, N, M, k, bip, bias):
    from gkgnet_amd import ops
    gen = torch.Generator().manual_seed(B * 1000 + N + 1)
    x = torch.randn(B, C, N, generator=gen)
    y = torch.randn(B, C, M, generator=gen) if bip else None
    idx = _random_graph(B, N, M if bip else N, k, gen)
    w = torch.randn(2 * C, generator=gen) * 0.5
    bv = torch.tensor([0.3]) if bias else None
    g = torch.randn(B, C, N, generator=gen)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yd = None if y is None else y.double().requires_grad_(True)
    bd = None if bv is None else bv.double().requires_grad_(True)
    sd = xd if yd is None else yd
    xj = _gather64(sd, idx)
    e = torch.einsum("c,bcn->bn", wd[:C], xd)[..., None] + torch.einsum("c,bcnk->bnk", wd[C:], xj)
    if bd is not None:
        e = e + bd
    p = torch.softmax(e, -1)
    want = (p[:, None] * xj).sum(-1)
    want.backward(g.double())
    xc, wc = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    yc = None if y is None else y.cuda().requires_grad_(True)
    bc = None if bv is None else bv.cuda().requires_grad_(True)
    got = ops.gat_aggregate(xc, idx.cuda(), wc, bc, yc)
    got.backward(g.cuda())
    assert torch.allclose(got.double().cpu(), want, atol=1e-5, rtol=1e-5)
    assert torch.allclose(xc.grad.double().cpu(), xd.grad, atol=1e-5, rtol=1e-4)
    if bip:
        assert torch.allclose(yc.grad.double().cpu(), yd.grad, atol=1e-5, rtol=1e-4)
    assert torch.allclose(wc.grad[C:].double().cpu(), wd.grad[C:], atol=1e-4, rtol=1e-4)
    assert torch.allclose(wc.grad[:C].double().cpu(), wd.grad[:C], atol=1e-4)          # exactly 0 up to rounding
    if bias:
        assert abs(float(bc.grad) - float(bd.grad)) < 1e-4


def test_ops_reject_bad_arguments():
    from gkgnet_amd import _lib, ops
    x = torch.randn(2, 8, 10, device="cuda")
    idx = torch.zeros(2, 10, 3, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.GkgError):
        ops.gin_aggregate(x.cpu(), idx.cpu(), torch.zeros(1))
    with pytest.raises(_lib.GkgError):
        ops.gin_aggregate(x.half(), idx, torch.zeros(1, device="cuda"))
    with pytest.raises(_lib.GkgError):
        ops.gat_aggregate(x, idx, torch.zeros(8, device="cuda"))            # needs 2C weights
    lib = _lib.load()
    assert lib.gkg_gin_fwd(None, None, None, None, None, 1, 1, 1, 1, 1, None) == -1
    assert lib.gkg_gin_fwd(x.data_ptr(), None, idx.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 8, 10, 10, 3, None) == -2
    assert lib.gkg_gat_bwd(x.data_ptr(), x.data_ptr(), None, idx.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, None,
                           None, 2, 8, 10, 10, 3, x.data_ptr(), 16, None) == -4                  # workspace too small
    assert lib.gkg_gconv_workspace_bytes(0, 8, 10, 10, 3) == 0


# ------------------------------------------------------------------------------------------- reference fixtures
@pytest.mark.parametrize("name", GRAPHER_CASES)
def test_grapher_fixture_forward_backward(name):
    meta, a = load_fixture(name)
    mod = make_grapher(meta)
    mod.load_state_dict(state_from(a))
    mod.cuda()
    x = _t(a["x"])
    assert mod.graph_conv.gconv._hip_plan(torch.zeros(1, meta["C"], 2, 1, device="cuda")) is not None
    cap = {}
    h = mod.graph_conv.register_forward_hook(lambda m, i, o: cap.update(edge=o[1].detach(), graph=o[0].detach()))
    mod.eval()
    with torch.no_grad():
        out_eval = mod(x)
    assert torch.allclose(out_eval, _t(a["out_eval"]), **TOL)
    mod.train()
    xg = x.clone().requires_grad_(True)
    out = mod(xg)
    h.remove()
    edge = cap["edge"].cpu().numpy()
    assert check_indices(edge[0], a["edge_index"][0], a["topd"], a["topi"], meta["dilation"]) == 0
    assert np.array_equal(edge[1], a["edge_index"][1])
    assert torch.allclose(cap["graph"], _t(a["graph"]), **TOL)
    assert torch.allclose(out, _t(a["out"]), **TOL)
    (out * _t(a["cot"])).sum().backward()
    assert torch.allclose(xg.grad, _t(a["dx"]), **TOL)
    _check_param_grads(mod, a)


@pytest.mark.parametrize("name", LABEL_CASES)
def test_label_fixture_forward_backward(name):
    meta, a = load_fixture(name)
    mod = make_label(meta)
    mod.load_state_dict(state_from(a))
    mod.cuda()
    e, feat = _t(a["e"]), _t(a["feat"])
    mod.eval()
    with torch.no_grad():
        out_eval, _ = mod(e, feat)
    assert torch.allclose(out_eval, _t(a["out_eval"]), **TOL)
    mod.train()
    eg, fg = e.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    out, idx = mod(eg, fg)
    assert check_indices(idx[0].cpu().numpy(), a["nn_idx"][0], a["topd"], a["topi"]) == 0
    assert torch.allclose(out, _t(a["out"]), **TOL)
    (out * _t(a["cot"])).sum().backward()
    assert torch.allclose(eg.grad, _t(a["de"]), **TOL)
    assert torch.allclose(fg.grad, _t(a["dfeat"]), **TOL)
    _check_param_grads(mod, a)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", GRAPHER_CASES + LABEL_CASES)
def test_fixture_gconv_replay_on_gpu(name, train):
    """graph_conv.gconv alone on the fixture's own inputs and graph, through the HIP path."""
    meta, a = load_fixture(name)
    mod = (make_grapher if meta["kind"] == "grapher" else make_label)(meta)
    mod.load_state_dict(state_from(a))
    gconv = mod.graph_conv.gconv.cuda().train(train)
    sfx = "" if train else "_eval"
    x = _t(a["gc_x" + sfx])
    y = _t(a["gc_y" + sfx]) if "gc_y" + sfx in a else None
    edge = _t(a["gc_edge" + sfx].astype(np.int64))
    assert gconv._hip_plan(x) is not None
    with torch.no_grad():
        out = gconv(x, edge, y)
    assert torch.allclose(out, _t(a["gc_out" + sfx]), atol=1e-4, rtol=1e-4), float((out - _t(a["gc_out" + sfx])).abs().max())


def _check_param_grads(mod, a):
    named = dict(mod.named_parameters())
    for k, g in grads_from(a).items():
        got = named[k].grad
        if got is None:
            assert float(g.abs().max()) < 2e-3, k
            continue
        assert torch.allclose(got, g.cuda(), atol=2e-3, rtol=2e-3), k


# ------------------------------------------------------------------------------------------- determinism
def test_backward_is_bit_identical_across_runs():
    from gkgnet_amd import ops
    gen = torch.Generator().manual_seed(5)
    B, C, N, M, k = 4, 64, 324, 81, 9
    x = torch.randn(B, C, N, generator=gen).cuda()
    y = torch.randn(B, C, M, generator=gen).cuda()
    idx = torch.randint(0, M, (B, N, k), generator=gen).cuda()
    idx_self = torch.randint(0, N, (B, N, k), generator=gen).cuda()
    g = torch.randn(B, C, N, generator=gen).cuda()
    w = (0.3 * torch.randn(2 * C, generator=gen)).cuda()

    def run(kind, src, nn_idx):
        xs = x.clone().requires_grad_(True)
        ss = None if src is None else src.clone().requires_grad_(True)
        if kind == "gin":
            p = torch.tensor([0.2], device="cuda", requires_grad=True)
            ops.gin_aggregate(xs, nn_idx, p, ss).backward(g)
            extra = [p.grad]
        else:
            p = w.clone().requires_grad_(True)
            b = torch.tensor([0.1], device="cuda", requires_grad=True)
            ops.gat_aggregate(xs, nn_idx, p, b, ss).backward(g)
            extra = [p.grad, b.grad]
        return [xs.grad] + ([] if ss is None else [ss.grad]) + extra

    for kind in ("gin", "gat"):
        for src, nn_idx in ((y, idx), (None, idx_self)):
            r1, r2 = run(kind, src, nn_idx), run(kind, src, nn_idx)
            for t1, t2 in zip(r1, r2):
                assert torch.equal(t1, t2), kind


# ------------------------------------------------------------------------------------------- memory
def _peaks(mod, x, edge, g):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = mod(x, edge)
    torch.cuda.synchronize()
    fwd = torch.cuda.max_memory_allocated() - base
    out.backward(g)
    torch.cuda.synchronize()
    total = torch.cuda.max_memory_allocated() - base
    del out
    x.grad = None
    for p in mod.parameters():
        p.grad = None
    return fwd, total


@pytest.mark.parametrize("conv", ["sage", "gin", "gat"])
def test_no_k_times_tensor(conv, local_bn):
    """B=8, C=320, N=324, k=9: the literal forms materialise (B, C, N, k) gathers, the HIP paths do not."""
    from gkgnet_amd import ops
    torch.manual_seed(3)
    B, C, N, k = 8, 320, 324, 9
    one = B * C * N * k * 4
    mod = _make(conv, C, 2 * C, "gelu", "batch").train()
    x = torch.randn(B, C, N, 1, device="cuda", requires_grad=True)
    edge = _edge(torch.randint(0, N, (B, N, k), device="cuda"))
    g = torch.randn(B, 2 * C, N, 1, device="cuda")
    assert mod._hip_plan(x) is not None
    _peaks(mod, x, edge, g)                                    # warm-up (allocator, library handles)
    hip_fwd, hip_total = _peaks(mod, x, edge, g)
    lit = _literal(copy.deepcopy(mod))
    _peaks(lit, x, edge, g)
    lit_fwd, lit_total = _peaks(lit, x, edge, g)
    print(f"{conv}: forward peak {hip_fwd / 2**20:.1f} MiB (literal {lit_fwd / 2**20:.1f}); fwd+bwd {hip_total / 2**20:.1f} MiB "
          f"(literal {lit_total / 2**20:.1f}); one (B,C,N,k) fp32 tensor = {one / 2**20:.1f} MiB")
    assert hip_total <= lit_total
    if conv != "gin":
        assert lit_fwd - hip_fwd >= one
        return
    # GIN: the literal gather is transient (summed at once); what follows it, nn on a (B, C, N) tensor, is the same on both
    # paths and overlaps the HIP path's peak.  Measure the aggregation itself: (B, C, N) out vs gather + sum.
    assert hip_fwd < lit_fwd
    xt, idx = x.detach().reshape(B, C, N), edge[0]
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    h = ops.gin_aggregate(xt, idx, mod.eps)
    agg_hip = torch.cuda.max_memory_allocated() - base
    del h
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    h = (1 + mod.eps) * x + torch.gather(xt, 2, idx.reshape(B, 1, N * k).expand(B, C, N * k)).reshape(B, C, N, k).sum(-1, keepdim=True)
    agg_lit = torch.cuda.max_memory_allocated() - base
    del h
    assert agg_lit - agg_hip >= one


# ------------------------------------------------------------------------------------------- multi-group, edge path
@pytest.mark.parametrize("conv", ["sage", "gin", "gat"])
def test_multi_group_forward_raises_like_the_reference(conv):
    from gkgnet_amd.grapher import Grapher
    mod = Grapher(32, 5, 1, conv, "gelu", "batch", True, False, 0.2, 1, n=36, relative_pos=True, use_multi_group=True,
                  num_group=2).cuda()
    mod.load_state_dict(mod.state_dict(), strict=True)
    with pytest.raises(RuntimeError):
        mod(torch.randn(2, 32, 6, 6, device="cuda"))


@pytest.mark.parametrize("norm_train", [None, "train", "eval"])
def test_edge_aggregate_null_qc_equals_zero_qc(norm_train, local_bn):
    from gkgnet_amd import ops
    from gkgnet_amd.layers import build_norm
    torch.manual_seed(11)
    B, O, N, M, k = 3, 16, 40, 29, 7
    qs = torch.randn(B, O, M, device="cuda")
    idx = torch.randint(0, M, (B, N, k), device="cuda")
    bias = (0.1 * torch.randn(O, device="cuda"))
    g = torch.randn(B, O, N, device="cuda")
    res = []
    for qc in (None, torch.zeros(B, O, N, device="cuda")):
        bn = None
        if norm_train is not None:
            torch.manual_seed(12)
            bn = build_norm(O).cuda().train(norm_train == "train")
            with torch.no_grad():
                bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.1)
                bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5)
        q = qs.clone().requires_grad_(True)
        b = bias.clone().requires_grad_(True)
        out = ops.edge_aggregate(q, qc, idx, b, None if bn is None else bn.weight, None if bn is None else bn.bias, bn,
                                 slice(0, O), ops.ACT_GELU)
        out.backward(g)
        res.append((out.detach(), q.grad, b.grad, bn))
    (o1, dq1, db1, bn1), (o2, dq2, db2, bn2) = res
    assert torch.equal(o1, o2)
    assert torch.allclose(dq1, dq2, atol=1e-6, rtol=1e-5)       # fp32 atomics: order-dependent rounding
    assert torch.allclose(db1, db2, atol=1e-5, rtol=1e-5)
    if bn1 is not None:
        assert torch.equal(bn1.running_mean, bn2.running_mean) and torch.equal(bn1.running_var, bn2.running_var)
        assert torch.allclose(bn1.weight.grad, bn2.weight.grad, atol=1e-5) and torch.allclose(bn1.bias.grad, bn2.bias.grad, atol=1e-5)


# ------------------------------------------------------------------------------------------- GIN / GAT beyond one workgroup
def _idx_randint(B, N, M, k):
    return torch.randint(0, M, (B, N, k), device="cuda")


def _module_vs_double(conv, B, C, N, M, k, bipartite, train, norm="batch", act="gelu", out=40):
    """The HIP path of a module against the SAME module's literal form evaluated in double on the same device and rounded to fp32
    (torch's fp32 train-mode BatchNorm backward is itself off by 1e-2 at N = 257 on this stack: EXPERIMENTS.md "EdgeConv gather
    kernels vs fp64"); tolerances are those of test_module_hip_matches_literal_form."""
    mod = _make(conv, C, out, act, norm)
    ref = _literal(copy.deepcopy(mod).double())
    mod.train(train); ref.train(train)
    x = torch.randn(B, C, N, 1, device="cuda", requires_grad=True)
    y = torch.randn(B, C, M, 1, device="cuda", requires_grad=True) if bipartite else None
    assert mod._hip_plan(x) is not None
    edge = _edge(_idx_randint(B, N, M if bipartite else N, k))
    outp = mod(x, edge, y)
    f = lambda t: t.float()                                                 # noqa: E731
    x2 = x.detach().double().requires_grad_(True)
    y2 = None if y is None else y.detach().double().requires_grad_(True)
    want = ref(x2, edge, y2)
    assert outp.shape == want.shape
    assert torch.allclose(outp, f(want), atol=2e-5, rtol=1e-5), float((outp - f(want)).abs().max())
    g = torch.randn_like(outp)
    outp.backward(g); want.backward(g.double())
    assert torch.allclose(x.grad, f(x2.grad), atol=5e-5, rtol=1e-4), float((x.grad - f(x2.grad)).abs().max())
    if bipartite:
        assert torch.allclose(y.grad, f(y2.grad), atol=5e-5, rtol=1e-4), float((y.grad - f(y2.grad)).abs().max())
    for (name, p), (_, q) in zip(mod.named_parameters(), ref.named_parameters()):
        gp = torch.zeros_like(p) if p.grad is None else p.grad
        gq = torch.zeros_like(p) if q.grad is None else f(q.grad)
        assert torch.allclose(gp, gq, atol=2e-4, rtol=1e-4), (name, float((gp - gq).abs().max()))
    for m, r in zip(mod.modules(), ref.modules()):
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            assert torch.allclose(m.running_mean, f(r.running_mean), atol=1e-5)
            assert torch.allclose(m.running_var, f(r.running_var), atol=1e-5, rtol=1e-5)
            assert int(m.num_batches_tracked) == int(r.num_batches_tracked)


@pytest.mark.parametrize("conv", ["gin", "gat"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("N,M,bipartite", [(257, 257, False), (300, 257, True)], ids=["n257-self", "n300-m257"])
def test_module_second_workgroup_matches_literal_form_in_double(conv, train, N, M, bipartite, local_bn):
    """N = 257: a second workgroup with one live thread; (N, M) = (300, 257): the scan's chunks of two.  randint lists (repeats)."""
    torch.manual_seed(7)
    _module_vs_double(conv, 3, 24, N, M, 6, bipartite, train)


@pytest.mark.parametrize("bipartite", [False, True])
def test_gat_single_image_agrees_with_the_literal_form(bipartite, local_bn, monkeypatch):
    """B = 1: the reference's ``.squeeze()`` drops the batch dimension along with the channel one; the result is the same function,
    and the HIP path (which is taken) must agree with it."""
    from gkgnet_amd import ops
    torch.manual_seed(7)
    real, spy = ops.gat_aggregate, []
    monkeypatch.setattr(ops, "gat_aggregate", lambda *a, **kw: (spy.append(1), real(*a, **kw))[1])
    _module_vs_double("gat", 1, 24, 50, 37, 6, bipartite, True)
    assert spy == [1], spy


@pytest.mark.parametrize("N,k", [(10, 1), (1, 4)], ids=["k1", "n1"])
def test_gat_k1_and_n1_take_the_literal_form(N, k, local_bn, monkeypatch):
    """At k = 1 the reference's squeeze() turns the softmax into one over nodes, at N = 1 into one over k with the node dimension
    gone: whatever that computes, the module computes it with the literal form and never calls the HIP attention."""
    from gkgnet_amd import ops
    torch.manual_seed(7)
    B, C = 1, 24
    mod = _make("gat", C, 40, "gelu", None)
    ref = _literal(copy.deepcopy(mod))
    x = torch.randn(B, C, N, 1, device="cuda")
    assert mod._hip_plan(x) is not None
    edge = _edge(_idx_randint(B, N, N, k))
    real, spy = ops.gat_aggregate, []
    monkeypatch.setattr(ops, "gat_aggregate", lambda *a, **kw: (spy.append(1), real(*a, **kw))[1])
    with torch.no_grad():
        got, want = mod(x, edge), ref(x, edge)
    assert spy == [] and torch.equal(got, want)
    mod2 = _make("gat", C, 40, "gelu", None)
    with torch.no_grad():
        mod2(torch.randn(B, C, 10, 1, device="cuda"), _edge(_idx_randint(B, 10, 10, 4)))
    assert spy == [1], "the spy sees the HIP attention when it runs"


def _grads_of(mod, x, y, edge, g):
    out = mod(x, edge, y)
    out.backward(g)
    return out.detach(), {n: p.grad for n, p in mod.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("conv", ["gin", "gat"])
def test_non_contiguous_inputs_give_the_same_bits(conv, local_bn):
    """x as a channels-last 4-D tensor, y as a transposed view: the wrappers make them contiguous; same bits as contiguous inputs."""
    torch.manual_seed(9)
    B, C, N, M, k = 2, 24, 70, 41, 5
    base = _make(conv, C, 40, "gelu", "batch").train()
    xl = torch.randn(B, N, 1, C, device="cuda", requires_grad=True)        # channels last
    yl = torch.randn(B, M, C, 1, device="cuda", requires_grad=True)
    x_nc, y_nc = xl.permute(0, 3, 1, 2), yl.transpose(1, 2)
    assert x_nc.shape == (B, C, N, 1) and y_nc.shape == (B, C, M, 1) and not x_nc.is_contiguous() and not y_nc.is_contiguous()
    xc = x_nc.detach().contiguous().requires_grad_(True)
    yc = y_nc.detach().contiguous().requires_grad_(True)
    edge = _edge(_idx_randint(B, N, M, k))
    g = torch.randn(B, 40, N, 1, device="cuda")
    o1, p1 = _grads_of(copy.deepcopy(base), xc, yc, edge, g)
    o2, p2 = _grads_of(copy.deepcopy(base), x_nc, y_nc, edge, g)
    assert torch.equal(o1, o2)
    assert torch.equal(xc.grad, xl.grad.permute(0, 3, 1, 2)) and torch.equal(yc.grad, yl.grad.transpose(1, 2))
    assert p1.keys() == p2.keys() and all(torch.equal(p1[n], p2[n]) for n in p1)


@pytest.mark.parametrize("conv", ["gin", "gat"])
@pytest.mark.parametrize("bipartite", [False, True])
def test_partial_grad_requests_equal_the_all_grad_run(conv, bipartite, local_bn):
    """Only the parameters require grad, and only the inputs do (geps / da / dbias are then not requested from the kernels):
    every gradient that is produced equals the all-grad run bit for bit."""
    torch.manual_seed(10)
    B, C, N, M, k = 2, 24, 70, 41, 5
    base = _make(conv, C, 40, "gelu", "batch").train()
    x0 = torch.randn(B, C, N, 1, device="cuda")
    y0 = torch.randn(B, C, M, 1, device="cuda") if bipartite else None
    edge = _edge(_idx_randint(B, N, M if bipartite else N, k))
    g = torch.randn(B, 40, N, 1, device="cuda")
    leaf = lambda t, on: None if t is None else t.clone().requires_grad_(on)    # noqa: E731
    xa, ya = leaf(x0, True), leaf(y0, True)
    o_all, p_all = _grads_of(copy.deepcopy(base), xa, ya, edge, g)
    assert p_all and all(bool(torch.isfinite(v).all()) for v in p_all.values())
    if conv == "gin":
        assert "eps" in p_all
    else:
        assert "a.weight" in p_all and "a.bias" in p_all
    xp, yp = leaf(x0, False), leaf(y0, False)
    o_par, p_par = _grads_of(copy.deepcopy(base), xp, yp, edge, g)
    assert torch.equal(o_all, o_par) and xp.grad is None
    assert p_par.keys() == p_all.keys() and all(torch.equal(p_par[n], p_all[n]) for n in p_all)
    xi, yi = leaf(x0, True), leaf(y0, True)
    o_in, p_in = _grads_of(copy.deepcopy(base).requires_grad_(False), xi, yi, edge, g)
    assert torch.equal(o_all, o_in) and p_in == {}
    assert torch.equal(xi.grad, xa.grad) and (not bipartite or torch.equal(yi.grad, ya.grad))


@pytest.mark.parametrize("kind", ["gin", "gat"])
def test_forward_and_backward_replay_from_a_captured_graph(kind):
    """One forward + backward of the operator, bipartite (2, 8, 300, 81, 5), captured after a warm-up on a side stream (one stream:
    no parallel branches) and replayed twice: outputs and gradients equal the eager run bit for bit."""
    from gkgnet_amd import ops
    gen = torch.Generator().manual_seed(21)
    B, C, N, M, k = 2, 8, 300, 81, 5
    x = torch.randn(B, C, N, generator=gen).cuda().requires_grad_(True)
    y = torch.randn(B, C, M, generator=gen).cuda().requires_grad_(True)
    idx = torch.randint(0, M, (B, N, k), generator=gen).cuda()
    g = torch.randn(B, C, N, generator=gen).cuda()
    if kind == "gin":
        params = [torch.tensor([0.2], device="cuda", requires_grad=True)]
        run = lambda: ops.gin_aggregate(x, idx, params[0], y)                # noqa: E731
    else:
        params = [(0.3 * torch.randn(2 * C, generator=gen)).cuda().requires_grad_(True), torch.tensor([0.1], device="cuda", requires_grad=True)]
        run = lambda: ops.gat_aggregate(x, idx, params[0], params[1], y)     # noqa: E731

    def step():
        out = run()
        return [out, *torch.autograd.grad(out, [x, y, *params], g)]

    eager = [t.detach().clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for turn in range(2):
        for t in static:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(static, eager):
            assert torch.equal(got.detach(), want), (kind, turn)
