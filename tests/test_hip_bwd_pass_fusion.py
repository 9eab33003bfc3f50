"""Round 8: backward passes folded into their producers (GKG_DISABLE=bwd_fuse switches all three off).

A. gkg_linear_dgrad_x6_nchw — the input-gradient GEMM stores (B, C, N) itself (csrc/gkg_gemm_x6.hip X6_STORE_NCHW): the bits of
   gkg_linear_dgrad_x6_sk + gkg_tm_affine_to_nchw (a pure re-layout).
B. gkg_nchw_to_tm_add_bnstats — the NCHW -> token-major (+ add) pass also takes the BN backward statistics of the layer whose
   upstream gradient it writes: g has the bits of gkg_nchw_to_tm_add; dY / dgamma / dbeta through gkg_bn_bwd_apply_from_sums agree
   with the two-pass gkg_bn_bwd_atomic to the rule tests/test_hip_bn_epilogue.py applies (the fp32 partial sums follow another
   partition of the rows): max abs difference <= 2e-4 * max(1, max |ref|).
C. gkg_mr_bwd_tm_bnstats — the aggregation's scatter also takes the statistics of the BN in front of it: gx / gsrc have the bits
   of gkg_mr_bwd_tm (self graph 18 x 18, G = 4, k = 9: the streaming form; label graph, 80 queries over 324 keys: the two-sweep
   form); statistics as in B; an inf in the gradient leaves the same outputs non-finite in both forms.
Blocks: Grapher + GrapherLabel (driver and composition), bwd_fuse on vs off."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _close(a, b, tol=2e-4):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _planes(lib, w, nb, cout, cin, kperm=0):
    pf = torch.empty(lib.gkg_x6_planes_bytes(cin, cout, nb, 0), dtype=torch.uint8, device="cuda")
    pd = torch.empty(lib.gkg_x6_planes_bytes(cin, cout, nb, 1), dtype=torch.uint8, device="cuda")
    host = ctypes.create_string_buffer(lib.gkg_x6_prep_desc_bytes())
    units = lib.gkg_x6_prep_desc_fill(host, 0, w.data_ptr(), pf.data_ptr(), pd.data_ptr(), cin, cout, nb, 0, kperm)
    assert units > 0
    descs = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).cuda()
    assert lib.gkg_x6_prep_weights(descs.data_ptr(), 1, units, None) == 0
    torch.cuda.synchronize()
    return pf, pd


# ---------------------------------------------------------------------------------------------------------------- A
# (B, N, cin, cout): cfg2's fc1 (R = 10 368, 320 -> 320); ragged rows (R = 5 196, R % 128 = 76, N % 4 == 0); a width that leaves a
# partial column tile (336 = 5 x 64 + 16); a single 32-column-block tile width (C = 64: the NI = 1 form); N % 4 != 0 and a short
# matrix (the two-launch fallbacks)
A_SHAPES = [(32, 324, 320, 320), (3, 1732, 320, 320), (8, 648, 336, 320), (48, 144, 64, 64), (64, 81, 320, 320), (4, 324, 320, 320)]


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("B,N,cin,cout", A_SHAPES)
def test_a_dgrad_stores_nchw_with_the_bits_of_the_two_launch_form(B, N, cin, cout, with_res):
    from gkgnet_amd import _lib, fused
    from gkgnet_amd.ops import _ptr, _stream
    lib = _lib.load()
    R = B * N
    gen = torch.Generator(device="cuda").manual_seed(R + cin)
    w = torch.randn(1, cout, cin, device="cuda", generator=gen) / cout ** 0.5
    dy = torch.randn(R, cout, device="cuda", generator=gen)
    res = torch.randn(R, cin, device="cuda", generator=gen) if with_res else None
    _, pd = _planes(lib, w, 1, cout, cin)
    sk = fused._sk_ws(dy.device)
    dxt = torch.full((R, cin), float("nan"), device="cuda")
    want = torch.full((B, cin, N), float("nan"), device="cuda")
    _lib.check(lib.gkg_linear_dgrad_x6_sk(_ptr(dy), cout, R * cout, _ptr(pd), _ptr(dxt), R, cin, cout, 1, _ptr(res), _ptr(sk), sk.numel(),
                                          0, 0, 0, _stream()), "gkg_linear_dgrad_x6_sk")
    _lib.check(lib.gkg_tm_affine_to_nchw(_ptr(dxt), None, None, None, _ptr(want), B, cin, N, None, _stream()), "gkg_tm_affine_to_nchw")
    got = torch.full((B, cin, N), float("nan"), device="cuda")
    scratch = torch.full((R, cin), float("nan"), device="cuda")
    _lib.check(lib.gkg_linear_dgrad_x6_nchw(_ptr(dy), cout, _ptr(pd), _ptr(got), _ptr(scratch), R, cin, cout, _ptr(res), B, N, _ptr(sk),
                                            sk.numel(), 0, _stream()), "gkg_linear_dgrad_x6_nchw")
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
    one_launch = N % 4 == 0 and R > 4096
    assert bool(torch.isnan(scratch).all()) == one_launch         # the scratch is touched by the two-launch form only


# ---------------------------------------------------------------------------------------------------------------- B
def _bn_case(R, C, gen):
    Y = torch.randn(R, C, device="cuda", generator=gen) * 1.5 + 0.3
    mean = Y.mean(0)
    invstd = 1.0 / torch.sqrt(Y.var(0, unbiased=False) + 1e-5)
    gamma = torch.rand(C, device="cuda", generator=gen) + 0.5
    a = gamma * invstd
    c = torch.randn(C, device="cuda", generator=gen) - mean * a
    return Y, mean.contiguous(), invstd.contiguous(), a.contiguous(), c.contiguous()


def _two_pass(lib, g, Y, a, c, mean, invstd, R, C):
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    dY, dgamma, dbeta = torch.empty_like(Y), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    sums = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    _lib.check(lib.gkg_bn_bwd_atomic(_ptr(g), _ptr(Y), _ptr(a), _ptr(c), _ptr(mean), _ptr(invstd), _ptr(dY), _ptr(dgamma), _ptr(dbeta),
                                     R, C, 1, C, 0, 0, _ptr(sums), None, 0, _stream()), "gkg_bn_bwd_atomic")
    return dY, dgamma, dbeta


def _apply_only(lib, g, Y, a, c, mean, invstd, R, C, sums):
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    dY, dgamma, dbeta = torch.empty_like(Y), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    _lib.check(lib.gkg_bn_bwd_apply_from_sums(_ptr(g), _ptr(Y), _ptr(a), _ptr(c), _ptr(mean), _ptr(invstd), _ptr(dY), _ptr(dgamma),
                                              _ptr(dbeta), R, C, 1, C, 0, 0, _ptr(sums), None, 0, _stream()), "gkg_bn_bwd_apply_from_sums")
    return dY, dgamma, dbeta


@pytest.mark.parametrize("with_add", [True, False])
@pytest.mark.parametrize("B,C,N", [(32, 320, 324), (3, 72, 50), (5, 64, 129)])
def test_b_relayout_pass_takes_the_bn_backward_statistics(B, C, N, with_add):
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    lib = _lib.load()
    R = B * N
    gen = torch.Generator(device="cuda").manual_seed(7 * R + C)
    x = torch.randn(B, C, N, device="cuda", generator=gen)
    add = torch.randn(R, C, device="cuda", generator=gen) if with_add else None
    Y, mean, invstd, a, c = _bn_case(R, C, gen)
    want_g = torch.empty(R, C, device="cuda")
    if with_add:
        _lib.check(lib.gkg_nchw_to_tm_add(_ptr(x), _ptr(add), _ptr(want_g), B, C, N, _stream()), "gkg_nchw_to_tm_add")
    else:
        _lib.check(lib.gkg_nchw_to_tm(_ptr(x), _ptr(want_g), B, C, N, _lib.F32, None, _stream()), "gkg_nchw_to_tm")
    ref = _two_pass(lib, want_g, Y, a, c, mean, invstd, R, C)
    g = torch.full((R, C), float("nan"), device="cuda")
    sums = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    _lib.check(lib.gkg_nchw_to_tm_add_bnstats(_ptr(x), _ptr(add), _ptr(g), _ptr(Y), _ptr(mean), _ptr(invstd), _ptr(sums), B, C, N,
                                              _stream()), "gkg_nchw_to_tm_add_bnstats")
    got = _apply_only(lib, g, Y, a, c, mean, invstd, R, C, sums)
    torch.cuda.synchronize()
    assert torch.equal(g, want_g)
    for name, u, v in zip(("dY", "dgamma", "dbeta"), got, ref):
        print(name, "max abs diff", float((u - v).abs().max()), "max |ref|", float(v.abs().max()))
        assert _close(u, v), name


@pytest.mark.parametrize("B,C,N", [(32, 320, 324), (5, 64, 129)])
def test_b_the_two_pass_side_of_the_comparison_ends_at_fp64(B, C, N):
    """Part B compares the fused form with gkg_nchw_to_tm_add + gkg_bn_bwd_atomic: kernel against kernel.  Here that two-launch side
    is held to the fp64 reference (tests/dense_ref.py) under the bar of tests/test_hip_dense_fp64.py, and so is the fused side."""
    from dense_ref import nchw_to_tm
    from test_hip_dense_fp64 import Bars, check_bn_bwd
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    lib = _lib.load()
    R = B * N
    gen = torch.Generator(device="cuda").manual_seed(7 * R + C)
    x = torch.randn(B, C, N, device="cuda", generator=gen)
    add = torch.randn(R, C, device="cuda", generator=gen)
    Y, mean, invstd, a, c = _bn_case(R, C, gen)
    g = torch.full((R, C), float("nan"), device="cuda")
    _lib.check(lib.gkg_nchw_to_tm_add(_ptr(x), _ptr(add), _ptr(g), B, C, N, _stream()), "gkg_nchw_to_tm_add")
    two = _two_pass(lib, g, Y, a, c, mean, invstd, R, C)
    g1 = torch.full((R, C), float("nan"), device="cuda")
    sums = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    _lib.check(lib.gkg_nchw_to_tm_add_bnstats(_ptr(x), _ptr(add), _ptr(g1), _ptr(Y), _ptr(mean), _ptr(invstd), _ptr(sums), B, C, N,
                                              _stream()), "gkg_nchw_to_tm_add_bnstats")
    fused_ = _apply_only(lib, g1, Y, a, c, mean, invstd, R, C, sums)
    torch.cuda.synchronize()
    assert torch.equal(g, nchw_to_tm(x, None, add))                    # a permutation and one fp32 add: correctly rounded on both sides
    for side, (dY, dgamma, dbeta) in (("two-pass", two), ("fused", fused_)):
        bars = Bars(f"pass_fusion B {side} B{B} C{C} N{N}")
        check_bn_bwd(bars, g[None], Y[None], a[None], c[None], mean[None], invstd[None], 0, dY, dgamma, dbeta)
        bars.done()


# ---------------------------------------------------------------------------------------------------------------- C
def _mr_case(B, G, c, N, M, gen, inf_at=None):
    C = G * c
    g = torch.randn(B * N, 2 * C, device="cuda", generator=gen)
    if inf_at is not None:
        g.view(-1)[inf_at] = float("inf")
    arg = torch.randint(0, M, (B, N, C), device="cuda", generator=gen).to(torch.int16)
    return g, arg


def _mr_both(lib, g, arg, B, G, c, N, M, k, self_graph, Y, mean, invstd):
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    C = G * c
    outs = []
    for fused_stats in (False, True):
        gx = torch.full((B, N, C), float("nan"), device="cuda")
        gs = None if self_graph else torch.full((B, M, C), float("nan"), device="cuda")
        sums = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
        if fused_stats:
            assert lib.gkg_mr_bwd_tm_bnstats_supported(B, G, c, N, M, k, 1, 1, 1 if self_graph else 0, 0) == 1
            _lib.check(lib.gkg_mr_bwd_tm_bnstats(_ptr(g), None, _ptr(arg), _ptr(gx), _ptr(gs), B, G, c, N, M, k, 1, 1, 0, _ptr(Y), _ptr(mean),
                                                 _ptr(invstd), _ptr(sums), _stream()), "gkg_mr_bwd_tm_bnstats")
        else:
            _lib.check(lib.gkg_mr_bwd_tm(_ptr(g), None, _ptr(arg), _ptr(gx), _ptr(gs), B, G, c, N, M, k, 1, 1, 0, _stream()), "gkg_mr_bwd_tm")
        outs.append((gx, gs, sums))
    return outs


# self graph 18 x 18 (streaming form), the label graph 80 over 324 (two-sweep form), a short self graph (two-sweep form, self) and
# a long bipartite one (streaming form, bipartite)
C_SHAPES = [(32, 4, 80, 324, 324, True), (32, 4, 80, 80, 324, False), (6, 2, 32, 144, 144, True), (4, 2, 40, 400, 100, False)]


@pytest.mark.parametrize("B,G,c,N,M,self_graph", C_SHAPES)
def test_c_scatter_takes_the_bn_backward_statistics(B, G, c, N, M, self_graph):
    from gkgnet_amd import _lib
    lib = _lib.load()
    C, R, k = G * c, B * N, 9
    gen = torch.Generator(device="cuda").manual_seed(R + M)
    g, arg = _mr_case(B, G, c, N, M, gen)
    Y, mean, invstd, a, cc = _bn_case(R, C, gen)
    (gx0, gs0, _), (gx1, gs1, sums) = _mr_both(lib, g, arg, B, G, c, N, M, k, self_graph, Y, mean, invstd)
    ref = _two_pass(lib, gx0.view(R, C), Y, a, cc, mean, invstd, R, C)
    got = _apply_only(lib, gx1.view(R, C), Y, a, cc, mean, invstd, R, C, sums)
    torch.cuda.synchronize()
    assert torch.isfinite(gx0).all()
    assert torch.equal(gx1, gx0)
    assert self_graph or torch.equal(gs1, gs0)
    for name, u, v in zip(("dY", "dgamma", "dbeta"), got, ref):
        print(name, "max abs diff", float((u - v).abs().max()), "max |ref|", float(v.abs().max()))
        assert _close(u, v), name


@pytest.mark.parametrize("B,G,c,N,M,self_graph", C_SHAPES[:2])
def test_c_an_inf_in_the_gradient_leaves_the_same_outputs_non_finite(B, G, c, N, M, self_graph):
    from gkgnet_amd import _lib
    lib = _lib.load()
    C, R, k = G * c, B * N, 9
    gen = torch.Generator(device="cuda").manual_seed(R + M + 1)
    # row 5 of image 1, the m half of the first channel chunk of the XM gradient layout
    g, arg = _mr_case(B, G, c, N, M, gen, inf_at=(N + 5) * 2 * C + C // 4 + 3)
    Y, mean, invstd, a, cc = _bn_case(R, C, gen)
    (gx0, gs0, _), (gx1, gs1, sums) = _mr_both(lib, g, arg, B, G, c, N, M, k, self_graph, Y, mean, invstd)
    ref = _two_pass(lib, gx0.view(R, C), Y, a, cc, mean, invstd, R, C)
    got = _apply_only(lib, gx1.view(R, C), Y, a, cc, mean, invstd, R, C, sums)
    torch.cuda.synchronize()
    assert not torch.isfinite(gx0).all()
    fin = torch.isfinite(gx0)
    # (the chunk that holds the inf is scattered with fp32 LDS atomics, whose order is run-dependent: its finite values agree
    # to rounding, like two runs of gkg_mr_bwd_tm itself)
    assert torch.equal(torch.isfinite(gx1), fin) and _close(gx1[fin], gx0[fin], 1e-5)
    if not self_graph:
        fs = torch.isfinite(gs0)
        assert not fs.all() and torch.equal(torch.isfinite(gs1), fs) and _close(gs1[fs], gs0[fs], 1e-5)
    for name, u, v in zip(("dY", "dgamma", "dbeta"), got, ref):
        assert not torch.isfinite(v).all(), name
        assert torch.equal(torch.isfinite(u), torch.isfinite(v)), name
        ok = torch.isfinite(v)
        assert _close(u[ok], v[ok]), name


def test_c_other_scatter_forms_are_reported_unsupported():
    from gkgnet_amd import _lib
    lib = _lib.load()
    assert lib.gkg_mr_bwd_tm_bnstats_supported(32, 4, 80, 324, 324, 9, 1, 1, 1, 0) == 1
    assert lib.gkg_mr_bwd_tm_bnstats_supported(32, 4, 80, 324, 324, 9, 0, 1, 1, 0) == 0                        # mode 0
    assert lib.gkg_mr_bwd_tm_bnstats_supported(32, 4, 80, 324, 324, 9, 1, 1, 1, _lib.MR_FP32_ATOMICS) == 0    # fp32 atomics
    assert lib.gkg_mr_bwd_tm_bnstats_supported(2, 2, 40, 20736, 1296, 9, 1, 1, 0, 0) == 0                      # long sweep, pooled keys
    assert lib.gkg_mr_bwd_tm_bnstats_supported(2, 4, 80, 100, 90000, 9, 1, 1, 0, 0) == 0                       # image beyond LDS


# ---------------------------------------------------------------------------------------------------------------- blocks
def _count(monkeypatch, lib, fused):
    """Calls of the new entry points: through the composition's helpers, and — the driver issues them from C — through the
    descriptors' bwd_flags at the two block-backward calls."""
    n = {"mr": 0, "relayout": 0, "drv_on": 0, "drv_off": 0}
    r_mr, r_re = lib.gkg_mr_bwd_tm_bnstats, lib.gkg_nchw_to_tm_add_bnstats
    monkeypatch.setattr(lib, "gkg_mr_bwd_tm_bnstats", lambda *a: (n.__setitem__("mr", n["mr"] + 1), r_mr(*a))[1])
    monkeypatch.setattr(lib, "gkg_nchw_to_tm_add_bnstats", lambda *a: (n.__setitem__("relayout", n["relayout"] + 1), r_re(*a))[1])
    for name in ("gkg_grapher_bwd", "gkg_grapher_label_bwd"):
        real = getattr(lib, name)

        def wrapped(d, wq, st, real=real):
            key = "drv_off" if d._obj.bwd_flags & 1 else "drv_on"
            n[key] += 1
            return real(d, wq, st)
        monkeypatch.setattr(lib, name, wrapped)
    return n


def _run_pair(monkeypatch, driver, on, C=64, H=14, L=20, B=24, G=2):
    from gkgnet_amd import _lib, block, fused
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    monkeypatch.setattr(block, "ENABLED", driver)
    monkeypatch.setattr(fused, "BWD_FUSE", on)
    block._PLANS.clear()
    torch.manual_seed(21)
    g = Grapher(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=True, use_multi_group=True,
                num_group=G).cuda().train()
    gl = GrapherLabel(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=False, num_nodes=L,
                      use_multi_group=True, num_group=G).cuda().train()
    params = list(g.parameters()) + list(gl.parameters())
    gen = torch.Generator(device="cuda").manual_seed(5)
    steps = []
    for step in range(3):                                # from the second step on the Grapher hands out both layouts
        x = torch.randn(B, C, H, H, device="cuda", generator=gen).requires_grad_(True)
        e = torch.randn(B, L, C, device="cuda", generator=gen).requires_grad_(True)
        cx, ce = torch.randn(B, C, H, H, device="cuda", generator=gen), torch.randn(B, L, C, device="cuda", generator=gen)
        for p in params:
            p.grad = None
        out = g(x)
        e2, edge = gl(e, out)
        torch.autograd.backward([out, e2], [cx, ce])
        torch.cuda.synchronize()
        steps.append(dict(out=out.detach().clone(), e2=e2.detach().clone(), edge=edge.clone(), dx=x.grad.clone(), de=e.grad.clone(),
                          grads=[None if p.grad is None else p.grad.clone() for p in params]))
    return steps


def _forward_equal(on, off):
    return all(torch.equal(a[key], b[key]) for a, b in zip(on, off) for key in ("out", "e2", "edge"))


@pytest.mark.parametrize("driver", [True, False])
def test_blocks_bwd_fuse_on_matches_off(driver, monkeypatch):
    """The forward does not depend on the switch: outputs and the graph must be the same bits.  (Two runs of the SAME path can
    differ in one BN channel's saved mean when its fp64 atomic sum lands on an fp32 rounding tie — tests/test_hip_block_driver.py —
    so a pair that differs is repeated, as there; a real difference would show in every pair.)"""
    from gkgnet_amd import _lib, block, fused
    lib = _lib.load()
    n = _count(monkeypatch, lib, fused)
    for attempt in range(4):
        for key in n:
            n[key] = 0
        on = _run_pair(monkeypatch, driver, True)
        n_on = dict(n)
        off = _run_pair(monkeypatch, driver, False)
        if driver:
            assert n_on["drv_on"] == 6 and n_on["drv_off"] == 0 and n["drv_off"] == 6 and n["drv_on"] == 6
        else:
            # per step: the scatters of both blocks, the re-layout pass of the Grapher's output gradient
            assert n_on["mr"] == 6 and n_on["relayout"] == 3 and n_on["drv_on"] == 0
            assert n["mr"] == 6 and n["relayout"] == 3                  # ... and none of them with bwd_fuse off
        if _forward_equal(on, off):
            break
    assert _forward_equal(on, off)
    for step, (a, b) in enumerate(zip(on, off)):
        for key in ("dx", "de"):
            print(step, key, float((a[key] - b[key]).abs().max()), float(b[key].abs().max()))
            assert _close(a[key], b[key]), (step, key)
        for u, v in zip(a["grads"], b["grads"]):
            assert (u is None) == (v is None)
            if u is not None:
                assert _close(u, v), step


def test_a_second_consumer_of_fc1_output_falls_back_cleanly(monkeypatch):
    """Another use of fc1's output adds a second gradient to the one the scatter took the statistics of: the layer must notice
    (the tensor it receives is not the one on the link), discard the sums and run its own statistics pass."""
    from gkgnet_amd import fused, layers
    layers.norm_cfg["type"] = "BN"
    B, N, C, G, k = 8, 324, 64, 2, 9
    R = B * N
    gen = torch.Generator(device="cuda").manual_seed(31)
    x0 = torch.randn(R, C, device="cuda", generator=gen)
    nn_idx = torch.randint(0, N, (B * G, N, k), device="cuda", generator=gen)
    for extra in ("after", "before", False):
        res = []
        for on in (True, False):
            monkeypatch.setattr(fused, "BWD_FUSE", on)
            torch.manual_seed(9)
            s1 = torch.nn.Sequential(torch.nn.Conv2d(C, C, 1), layers.build_norm(C)).cuda().train()
            s2 = torch.nn.Sequential(torch.nn.Conv2d(C, C, 1), layers.build_norm(C)).cuda().train()
            x = x0.clone().requires_grad_(True)
            h = fused._lin(x, s1, xm=(B, N))
            assert (getattr(h, "_gkg_mr_bn_link", None) is not None) == on
            side = (h * 0.5).sum() if extra == "before" else 0
            XM = fused._MaxRelativeTM.apply(h, None, nn_idx, G, 1, False)
            if extra == "after":
                side = (h * 0.5).sum()
            out = fused._lin(XM[:, :C].contiguous(), s2)          # a second BN layer behind: the scratch protocol must stay intact
            (out.square().sum() + XM.square().sum() + side).backward()
            torch.cuda.synchronize()
            res.append((x.grad.clone(), [p.grad.clone() for p in list(s1.parameters()) + list(s2.parameters()) if p.grad is not None]))
        (g1, p1), (g2, p2) = res
        assert _close(g1, g2, 5e-4), (extra, float((g1 - g2).abs().max()))
        assert len(p1) == len(p2) and all(_close(u, v, 5e-4) for u, v in zip(p1, p2)), extra
