"""Round 9, part 1: the BN backward statistics of a layer whose upstream gradient an input-gradient GEMM writes are taken in that
GEMM's epilogue at every size (gkg_linear_dgrad_x6_bnbwd_sk: the short-matrix body gemm_x6_ks_kernel carries them too, a residual
is added in front of them), and the layer's backward runs gkg_bn_bwd_apply_from_sums only.  GKG_DISABLE=dgrad_stats /
GKG_BLOCK_NO_DGRAD_STATS: off.

Kernel level, per shape: dx has the BITS of gkg_linear_dgrad_x6_sk (same kernel body, same order of the contraction); dY / dgamma /
dbeta agree with the two-pass gkg_bn_bwd_atomic within the bound tests/test_hip_bwd_pass_fusion.py uses for the same effect (the
fp32 partial sums follow the producer's partition of the rows): max abs difference <= 2e-4 * max(1, max |ref|).  Measured on an
MI355X (printed by the test): at most 1.8e-7 * max(1, max |ref|) over every case below.
Blocks: a Grapher + GrapherLabel pair through the driver and through the composition, part on: bit-identical to each other; on
vs off: to rounding."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-4


def _rel(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def _planes(lib, w, nb, cout, cin):
    pf = torch.empty(lib.gkg_x6_planes_bytes(cin, cout, nb, 0), dtype=torch.uint8, device="cuda")
    pd = torch.empty(lib.gkg_x6_planes_bytes(cin, cout, nb, 1), dtype=torch.uint8, device="cuda")
    host = ctypes.create_string_buffer(lib.gkg_x6_prep_desc_bytes())
    units = lib.gkg_x6_prep_desc_fill(host, 0, w.data_ptr(), pf.data_ptr(), pd.data_ptr(), cin, cout, nb, 0, 0)
    assert units > 0
    descs = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).cuda()
    assert lib.gkg_x6_prep_weights(descs.data_ptr(), 1, units, None) == 0
    torch.cuda.synchronize()
    return pf, pd


def _bn_case(R, pnb, pco, gen):
    """The producer layer h = act(BN(Y)), Y (pnb, R, pco): its saved tensors."""
    Y = torch.randn(pnb, R, pco, device="cuda", generator=gen) * 1.5 + 0.3
    mean = Y.mean(1)
    invstd = 1.0 / torch.sqrt(Y.var(1, unbiased=False) + 1e-5)
    gamma = torch.rand(pnb, pco, device="cuda", generator=gen) + 0.5
    a = gamma * invstd
    c = torch.randn(pnb, pco, device="cuda", generator=gen) * 0.3 - mean * a
    return Y, mean.reshape(-1).contiguous(), invstd.reshape(-1).contiguous(), a.reshape(-1).contiguous(), c.reshape(-1).contiguous()


# (R, cin = pnb * pco, cout, pnb, act, residual).  The four cfg2 folds: the label FFN fc1 BN from the FFN fc2 input gradient (tile
# body), the label fc2 BN from the FFN fc1 input gradient + residual (short-matrix body), the label / the Grapher grouped BN from
# fc2's input gradient (short-matrix / tile body).  Then: ragged last row blocks on both bodies (R % 32, R % 128 != 0), pnb in
# {1, 4}, act in {none, GELU}, with / without a residual, a column count that leaves a partial column tile (336), and a shape the
# tile body runs with the cross-workgroup split-K (512 x 1280 <- 320).
CASES = [
    (2560, 1280, 320, 1, 1, False),
    (2560, 320, 1280, 1, 0, True),
    (2560, 640, 320, 4, 1, False),
    (10368, 640, 320, 4, 1, False),
    (1003, 320, 96, 1, 0, True),
    (2571, 160, 64, 4, 1, True),
    (77, 336, 128, 1, 1, False),
    (5196, 192, 64, 1, 1, False),
    (4100, 336, 64, 4, 0, False),
    (512, 1280, 320, 1, 0, False),
]


@pytest.mark.parametrize("R,cin,cout,pnb,act,with_res", CASES)
def test_dgrad_epilogue_statistics_match_the_stand_alone_pass(R, cin, cout, pnb, act, with_res):
    from gkgnet_amd import _lib, fused
    from gkgnet_amd.ops import _ptr, _stream
    lib = _lib.load()
    pco = cin // pnb
    gen = torch.Generator(device="cuda").manual_seed(R + 3 * cin + cout)
    w = torch.randn(1, cout, cin, device="cuda", generator=gen) / cout ** 0.5
    dy = torch.randn(R, cout, device="cuda", generator=gen)
    res = torch.randn(R, cin, device="cuda", generator=gen) if with_res else None
    Y, mean, invstd, a, c = _bn_case(R, pnb, pco, gen)
    _, pd = _planes(lib, w, 1, cout, cin)
    sk = fused._sk_ws(dy.device)
    gbs = pco if pnb > 1 else 0
    # off: the plain input gradient, then the two-launch BN backward
    dx0 = torch.full((R, cin), float("nan"), device="cuda")
    _lib.check(lib.gkg_linear_dgrad_x6_sk(_ptr(dy), cout, R * cout, _ptr(pd), _ptr(dx0), R, cin, cout, 1, _ptr(res), _ptr(sk), sk.numel(),
                                          0, 0, 0, _stream()), "gkg_linear_dgrad_x6_sk")
    ref = torch.empty_like(Y), torch.empty(cin, device="cuda"), torch.empty(cin, device="cuda")
    sums0 = torch.zeros(2 * cin, dtype=torch.float64, device="cuda")
    _lib.check(lib.gkg_bn_bwd_atomic(_ptr(dx0), _ptr(Y), _ptr(a), _ptr(c), _ptr(mean), _ptr(invstd), _ptr(ref[0]), _ptr(ref[1]),
                                     _ptr(ref[2]), R, pco, pnb, cin, gbs, act, _ptr(sums0), None, 0, _stream()), "gkg_bn_bwd_atomic")
    # on: statistics in the GEMM's epilogue, then the apply pass only
    assert lib.gkg_linear_dgrad_x6_bnbwd_sk_supported(R, cin, 1 if with_res else 0, 1, 0) == 1
    dx1 = torch.full((R, cin), float("nan"), device="cuda")
    sums1 = torch.zeros(2 * cin, dtype=torch.float64, device="cuda")
    _lib.check(lib.gkg_linear_dgrad_x6_bnbwd_sk(_ptr(dy), cout, _ptr(pd), _ptr(dx1), R, cin, cout, _ptr(res), _ptr(Y), _ptr(a), _ptr(c),
                                                _ptr(mean), _ptr(invstd), _ptr(sums1), pnb, pco, act, _ptr(sk), sk.numel(), 0, _stream()),
               "gkg_linear_dgrad_x6_bnbwd_sk")
    got = torch.empty_like(Y), torch.empty(cin, device="cuda"), torch.empty(cin, device="cuda")
    _lib.check(lib.gkg_bn_bwd_apply_from_sums(_ptr(dx1), _ptr(Y), _ptr(a), _ptr(c), _ptr(mean), _ptr(invstd), _ptr(got[0]), _ptr(got[1]),
                                              _ptr(got[2]), R, pco, pnb, cin, gbs, act, _ptr(sums1), None, 0, _stream()),
               "gkg_bn_bwd_apply_from_sums")
    torch.cuda.synchronize()
    assert torch.isfinite(dx0).all()
    assert torch.equal(dx1, dx0)
    for name, u, v in zip(("dY", "dgamma", "dbeta"), got, ref):
        print(f"R={R} cin={cin} cout={cout} pnb={pnb} act={act} res={with_res} {name}: max abs diff / max(1, max |ref|) = {_rel(u, v):.3e}")
        assert torch.isfinite(u).all(), name
        assert _rel(u, v) <= TOL, name


@pytest.mark.parametrize("R,cin,cout,pnb,act,with_res", [(2571, 160, 64, 4, 1, True), (10368, 640, 320, 4, 1, False), (1003, 320, 96, 1, 0, True)])
def test_the_stand_alone_pass_of_the_comparison_ends_at_fp64(R, cin, cout, pnb, act, with_res):
    """The test above compares the epilogue statistics with the two-launch gkg_bn_bwd_atomic: kernel against kernel.  Here both
    sides' dY / dgamma / dbeta are held to the fp64 reference (tests/dense_ref.py) of the BN backward of the gradient dx the GEMM
    wrote, under the bar of tests/test_hip_dense_fp64.py."""
    from test_hip_dense_fp64 import Bars, check_bn_bwd
    from gkgnet_amd import _lib, fused
    from gkgnet_amd.ops import _ptr, _stream
    lib = _lib.load()
    pco = cin // pnb
    gen = torch.Generator(device="cuda").manual_seed(R + 3 * cin + cout)
    w = torch.randn(1, cout, cin, device="cuda", generator=gen) / cout ** 0.5
    dy = torch.randn(R, cout, device="cuda", generator=gen)
    res = torch.randn(R, cin, device="cuda", generator=gen) if with_res else None
    Y, mean, invstd, a, c = _bn_case(R, pnb, pco, gen)
    _, pd = _planes(lib, w, 1, cout, cin)
    sk = fused._sk_ws(dy.device)
    gbs = pco if pnb > 1 else 0
    dx = torch.full((R, cin), float("nan"), device="cuda")
    sums1 = torch.zeros(2 * cin, dtype=torch.float64, device="cuda")
    _lib.check(lib.gkg_linear_dgrad_x6_bnbwd_sk(_ptr(dy), cout, _ptr(pd), _ptr(dx), R, cin, cout, _ptr(res), _ptr(Y), _ptr(a), _ptr(c),
                                                _ptr(mean), _ptr(invstd), _ptr(sums1), pnb, pco, act, _ptr(sk), sk.numel(), 0, _stream()),
               "gkg_linear_dgrad_x6_bnbwd_sk")
    sides = {}
    for side in ("two-pass", "epilogue"):
        out = torch.full_like(Y, float("nan")), torch.full((cin,), float("nan"), device="cuda"), torch.full((cin,), float("nan"), device="cuda")
        if side == "two-pass":
            sums0 = torch.zeros(2 * cin, dtype=torch.float64, device="cuda")
            _lib.check(lib.gkg_bn_bwd_atomic(_ptr(dx), _ptr(Y), _ptr(a), _ptr(c), _ptr(mean), _ptr(invstd), *[_ptr(t) for t in out],
                                             R, pco, pnb, cin, gbs, act, _ptr(sums0), None, 0, _stream()), "gkg_bn_bwd_atomic")
        else:
            _lib.check(lib.gkg_bn_bwd_apply_from_sums(_ptr(dx), _ptr(Y), _ptr(a), _ptr(c), _ptr(mean), _ptr(invstd), *[_ptr(t) for t in out],
                                                      R, pco, pnb, cin, gbs, act, _ptr(sums1), None, 0, _stream()), "gkg_bn_bwd_apply_from_sums")
        sides[side] = out
    torch.cuda.synchronize()
    g = dx.view(R, pnb, pco).permute(1, 0, 2).contiguous()                # dout[q] = columns [q * pco, (q + 1) * pco) of dx
    per = lambda t: t.view(pnb, pco)      # noqa: E731
    for side, (dY, dgamma, dbeta) in sides.items():
        bars = Bars(f"dgrad_stats {side} R{R} cin{cin} pnb{pnb} act{act}")
        check_bn_bwd(bars, g, Y, per(a), per(c), per(mean), per(invstd), act, dY, per(dgamma), per(dbeta))
        bars.done()


def test_the_round_4_entry_point_is_the_sk_form_without_a_workspace():
    """gkg_linear_dgrad_x6_bnbwd (no workspace, no residual: the 128-row tile body whatever the shape) against
    gkg_linear_dgrad_x6_bnbwd_sk with a NULL workspace: the same dx bits, and the statistics to the bound above."""
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    lib = _lib.load()
    R, cin, cout, pnb, act = 2560, 640, 320, 4, 1
    pco = cin // pnb
    gen = torch.Generator(device="cuda").manual_seed(17)
    w = torch.randn(1, cout, cin, device="cuda", generator=gen) / cout ** 0.5
    dy = torch.randn(R, cout, device="cuda", generator=gen)
    Y, mean, invstd, a, c = _bn_case(R, pnb, pco, gen)
    _, pd = _planes(lib, w, 1, cout, cin)
    dx0, dx1 = torch.full((R, cin), float("nan"), device="cuda"), torch.full((R, cin), float("nan"), device="cuda")
    s0, s1 = (torch.zeros(2 * cin, dtype=torch.float64, device="cuda") for _ in range(2))
    _lib.check(lib.gkg_linear_dgrad_x6_bnbwd(_ptr(dy), cout, _ptr(pd), _ptr(dx0), R, cin, cout, _ptr(Y), _ptr(a), _ptr(c), _ptr(mean),
                                             _ptr(invstd), _ptr(s0), pnb, pco, act, _stream()), "gkg_linear_dgrad_x6_bnbwd")
    _lib.check(lib.gkg_linear_dgrad_x6_bnbwd_sk(_ptr(dy), cout, _ptr(pd), _ptr(dx1), R, cin, cout, None, _ptr(Y), _ptr(a), _ptr(c),
                                                _ptr(mean), _ptr(invstd), _ptr(s1), pnb, pco, act, None, 0, 0, _stream()),
               "gkg_linear_dgrad_x6_bnbwd_sk")
    torch.cuda.synchronize()
    assert torch.isfinite(dx0).all() and torch.equal(dx0, dx1)
    assert float(s0.abs().max()) > 0 and _rel(s0, s1) <= TOL


def test_a_residual_on_the_tile_body_is_reported_unsupported():
    from gkgnet_amd import _lib, fused
    from gkgnet_amd.ops import _ptr, _stream
    lib = _lib.load()
    assert lib.gkg_linear_dgrad_x6_bnbwd_sk_supported(10368, 320, 1, 1, 0) == 0          # too many rows for the short-matrix body
    assert lib.gkg_linear_dgrad_x6_bnbwd_sk_supported(2560, 1280, 1, 1, 0) == 0          # too many columns
    assert lib.gkg_linear_dgrad_x6_bnbwd_sk_supported(2560, 320, 1, 0, 0) == 0           # no workspace: the tile body
    assert lib.gkg_linear_dgrad_x6_bnbwd_sk_supported(2560, 320, 1, 1, _lib.X6_NO_KS) == 0
    assert lib.gkg_linear_dgrad_x6_bnbwd_sk_supported(2560, 320, 1, 1, 0) == 1
    assert lib.gkg_linear_dgrad_x6_bnbwd_sk_supported(10368, 640, 0, 1, 0) == 1
    R, cin, cout = 5000, 64, 64
    t = torch.zeros(R, cin, device="cuda")
    v = torch.zeros(cin, device="cuda")
    sums = torch.zeros(2 * cin, dtype=torch.float64, device="cuda")
    w = torch.zeros(1, cout, cin, device="cuda")
    _, pd = _planes(lib, w, 1, cout, cin)
    sk = fused._sk_ws(t.device)
    dx = torch.full((R, cin), float("nan"), device="cuda")
    rc = lib.gkg_linear_dgrad_x6_bnbwd_sk(_ptr(t), cout, _ptr(pd), _ptr(dx), R, cin, cout, _ptr(t), _ptr(t), _ptr(v), _ptr(v), _ptr(v),
                                          _ptr(v), _ptr(sums), 1, cin, 0, _ptr(sk), sk.numel(), 0, _stream())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED and bool(torch.isnan(dx).all())                    # nothing launched


# ---------------------------------------------------------------------------------------------------------------- blocks
def _run_pair(monkeypatch, driver, on, n, C=64, H=14, L=20, B=24, G=2):
    from gkgnet_amd import block, fused
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    monkeypatch.setattr(block, "ENABLED", driver)
    monkeypatch.setattr(fused, "DGRAD_STATS", on)
    block._PLANS.clear()
    for key in n:
        n[key] = 0
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
                          grads=[None if p.grad is None else p.grad.clone() for p in params],
                          names=[name for name, _ in list(g.named_parameters()) + list(gl.named_parameters())]))
    return steps, dict(n)


def _count(monkeypatch, lib):
    """Calls of the new entry point by the composition, and the descriptors' bwd_flags at the driver's two backward calls."""
    n = {"link": 0, "drv_on": 0, "drv_off": 0}
    real = lib.gkg_linear_dgrad_x6_bnbwd_sk
    monkeypatch.setattr(lib, "gkg_linear_dgrad_x6_bnbwd_sk", lambda *a: (n.__setitem__("link", n["link"] + 1), real(*a))[1])
    for name in ("gkg_grapher_bwd", "gkg_grapher_label_bwd"):
        realb = getattr(lib, name)

        def wrapped(d, wq, st, realb=realb):
            n["drv_off" if d._obj.bwd_flags & 3 else "drv_on"] += 1
            return realb(d, wq, st)
        monkeypatch.setattr(lib, name, wrapped)
    return n


def _first_difference(a_steps, b_steps):
    """Bit for bit, as tests/test_hip_block_driver.py: outputs, graph, input gradients; weight gradients (slabs added with fp32
    atomics) and BN parameter gradients (fp64-accumulated sums) to rounding."""
    for step, (a, b) in enumerate(zip(a_steps, b_steps)):
        for key in ("out", "e2", "edge", "dx", "de"):
            if not torch.equal(a[key], b[key]):
                return (step, key, float((a[key].float() - b[key].float()).abs().max()), int((a[key] != b[key]).sum()))
        for name, u, v in zip(a["names"], a["grads"], b["grads"]):
            if (u is None) != (v is None):
                return (step, name, "presence")
            if u is None:
                continue
            if u.dim() >= 2:
                ok = torch.allclose(u, v, rtol=1e-4, atol=1e-3 * float(v.abs().max()) + 1e-6)
            else:
                ok = torch.allclose(u, v, rtol=1e-5, atol=1e-5 * float(v.abs().max()) + 1e-7)
            if not ok:
                return (step, name)
    return None


def test_driver_and_composition_are_bit_identical_with_the_part_on(monkeypatch):
    """Both fold the same four statistics passes (the Grapher's grouped BN; the label block's FFN fc1, fc2 and grouped BN) into the
    same GEMM launches.  (A BN mean on an fp32 rounding tie can differ between two runs of the SAME path — see
    tests/test_hip_block_driver.py — so a pair that differs is repeated; a real difference shows in every pair.)"""
    from gkgnet_amd import _lib, block
    lib = _lib.load()
    n = _count(monkeypatch, lib)
    diff = None
    for attempt in range(4):
        drv, n_drv = _run_pair(monkeypatch, True, True, n)
        comp, n_comp = _run_pair(monkeypatch, False, True, n)
        assert n_drv == {"link": 0, "drv_on": 6, "drv_off": 0}
        assert n_comp == {"link": 12, "drv_on": 0, "drv_off": 0}          # per step: 1 in the Grapher, 3 in the label block
        diff = _first_difference(drv, comp)
        if diff is None:
            break
    assert diff is None, diff


@pytest.mark.parametrize("driver", [True, False])
def test_blocks_part_on_matches_off(driver, monkeypatch):
    from gkgnet_amd import _lib, block
    lib = _lib.load()
    n = _count(monkeypatch, lib)
    for attempt in range(4):
        on, n_on = _run_pair(monkeypatch, driver, True, n)
        off, n_off = _run_pair(monkeypatch, driver, False, n)
        assert n_off["link"] == 0 and n_off["drv_on"] == 0 and n_off["drv_off"] == (6 if driver else 0)
        assert (n_on["drv_on"], n_on["link"]) == ((6, 0) if driver else (0, 12))
        same_fwd = all(torch.equal(a[key], b[key]) for a, b in zip(on, off) for key in ("out", "e2", "edge"))
        if same_fwd:
            break
    assert same_fwd                                        # the forward does not depend on the switch
    for step, (a, b) in enumerate(zip(on, off)):
        for key in ("dx", "de"):
            print(step, key, f"{_rel(a[key], b[key]):.3e}")
            assert _rel(a[key], b[key]) <= TOL, (step, key)
        for name, u, v in zip(a["names"], a["grads"], b["grads"]):
            assert (u is None) == (v is None)
            if u is not None:
                assert _rel(u, v) <= TOL, (step, name)
