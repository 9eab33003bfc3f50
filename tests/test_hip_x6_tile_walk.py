"""Round 11: the tile-walk form of the 128-row projection kernel (csrc/gkg_gemm_x6_tile.h, gemm_x6_walk_kernel).  A launch of two
rounds of resident workgroups runs as one round of workgroups that each walk a static list of tiles, the rings carried from tile
to tile.  GKG_X6_FORCE_WALK takes the form at any size and its cap field bounds the grid, so a few hundred rows
reach every seam: several tiles per workgroup, a partial last row block and column tile, fewer K-steps than ring stages (the fetch
cursors then run more than one tile ahead), a K tail, the batch index folded into the list, and every epilogue.

Each case runs the same operands three times — forced walk on 8 workgroups, forced walk uncapped, GKG_X6_NO_WALK — and asserts
  * y / dx bit-identical between all three (same tile, same instruction order per accumulator),
  * the fp64 column sums within rtol 1e-12 of each other (the per-tile terms are the same; only the order of the atomics differs),
  * y / dx against fp64 at the bar of tests/test_hip_gemm_x6.py: error <= max(fp32 bmm error, 1.2e-7) relative to sum |a b|."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


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


def _rel(a, ref, scale):
    return float(((a.double() - ref).abs() / scale).max())


def _three_flags(_lib):
    """Forced walk on 8 workgroups, forced walk on the grid the rule picks, the one-tile form."""
    return (_lib.X6_FORCE_WALK | (1 << _lib.X6_WALK_CAP_SHIFT), _lib.X6_FORCE_WALK, _lib.X6_NO_WALK)


# (R, cin, cout, nb), 64-column tiles.  Row block u (batches folded in) belongs to XCD u % 8, so 8 workgroups walk:
#   (1100, 96, 160, 1)  9 row blocks x 3 column tiles: 6 tiles on XCD 0, 3 on the others; nk = 3 = the A ring's depth; last row
#                       block partial (1100 = 8 * 128 + 76), last column tile half used.  Its input gradient: nk = 5, 2 column tiles
#   (700, 32 | 64, 64)  nk = 1 and 2 on at most one tile per workgroup (6 row blocks on 8 XCDs): a stream that ends inside the
#                       prologue's five fetches
#   (2300, 32 | 64, 64) the same K on 18 row blocks: two or three tiles per workgroup, so that with nk < 3 the fetch cursors run
#                       two and three tiles ahead of the tile being computed (the 700-row shapes never cross a tile there)
#   (900, 40, 96, 1)    a K tail (40 = 32 + 8) on both tiles of every workgroup
#   (520, 160, 160, 4)  grouped: 20 (batch, row block) units, 9 or 6 tiles per workgroup across batch boundaries
SHAPES = [(1100, 96, 160, 1), (700, 32, 64, 1), (700, 64, 64, 1), (2300, 32, 64, 1), (2300, 64, 64, 1), (900, 40, 96, 1),
          (520, 160, 160, 4)]


@pytest.mark.parametrize("R,cin,cout,nb", SHAPES)
def test_walk_forward_statistics_store_and_dgrad_have_the_one_tile_bits(R, cin, cout, nb):
    from gkgnet_amd import _lib
    lib = _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(R * 7 + cin + cout)
    x = torch.randn(nb, R, cin, device="cuda", generator=gen) * 2 + 0.5
    w = torch.randn(nb, cout, cin, device="cuda", generator=gen) * 0.1
    dy = torch.randn(nb, R, cout, device="cuda", generator=gen)
    res = torch.randn(nb, R, cin, device="cuda", generator=gen)
    pf, pd = _planes(lib, w, nb, cout, cin)
    stats = torch.zeros(lib.gkg_linear_stats_doubles(), dtype=torch.float64, device="cuda")
    outs = []
    for flags in _three_flags(_lib):
        # no split-K workspace: the 128-row tile kernel whatever the size
        y = torch.full((nb, R, cout), float("nan"), device="cuda")           # BN-statistics epilogue
        stats.zero_()
        _lib.check(lib.gkg_linear_bn_fwd_x6_sk(x.data_ptr(), cin, R * cin, pf.data_ptr(), y.data_ptr(), R, cin, cout, nb, 2,
                                               *([None] * 10), 0.0, 0.0, stats.data_ptr(), None, 0, flags, None), "fwd + statistics")
        y0 = torch.full((nb, R, cout), float("nan"), device="cuda")          # plain store
        _lib.check(lib.gkg_linear_bn_fwd_x6_sk(x.data_ptr(), cin, R * cin, pf.data_ptr(), y0.data_ptr(), R, cin, cout, nb, 0,
                                               *([None] * 10), 0.0, 0.0, None, None, 0, flags, None), "fwd")
        dx = torch.full((nb, R, cin), float("nan"), device="cuda")           # store + residual
        _lib.check(lib.gkg_linear_dgrad_x6_sk(dy.data_ptr(), cout, R * cout, pd.data_ptr(), dx.data_ptr(), R, cin, cout, nb,
                                              res.data_ptr(), None, 0, 0, 0, flags, None), "dgrad")
        torch.cuda.synchronize()
        outs.append((y, y0, dx, stats[:nb * 2 * cout].clone()))
    y, y0, dx, st = outs[2]                                                  # the one-tile form
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    for yw, y0w, dxw, stw in outs[:2]:
        assert torch.equal(yw, y) and torch.equal(y0w, y0) and torch.equal(y0w, yw) and torch.equal(dxw, dx)
        torch.testing.assert_close(stw, st, rtol=1e-12, atol=0.0)
    ref_y = torch.bmm(x.double(), w.double().transpose(1, 2))
    ref_dx = torch.bmm(dy.double(), w.double()) + res.double()
    mag_y = torch.bmm(x.double().abs(), w.double().abs().transpose(1, 2)) + 1e-30
    mag_dx = torch.bmm(dy.double().abs(), w.double().abs()) + res.double().abs() + 1e-30
    e_y, e_dx = _rel(outs[0][0], ref_y, mag_y), _rel(outs[0][2], ref_dx, mag_dx)
    f_y = _rel(torch.bmm(x, w.transpose(1, 2)), ref_y, mag_y)
    f_dx = _rel(torch.baddbmm(res, dy, w), ref_dx, mag_dx)
    print(f"R={R} cin={cin} cout={cout} nb={nb}: y {e_y:.3e} (fp32 bmm {f_y:.3e}), dx {e_dx:.3e} (fp32 {f_dx:.3e})")
    assert e_y <= max(f_y, 1.2e-7) and e_dx <= max(f_dx, 1.2e-7), (e_y, f_y, e_dx, f_dx)
    sums = outs[0][3].view(nb, 2, cout)                                      # the epilogue's column sums: sum y, sum y^2
    assert torch.allclose(sums[:, 0], ref_y.sum(1), rtol=1e-6, atol=1e-3)
    assert torch.allclose(sums[:, 1], (ref_y * ref_y).sum(1), rtol=1e-5)


def test_walk_channel_major_store_across_image_boundaries():
    """gkg_linear_dgrad_x6_nchw, 2 images of 324 tokens (648 rows: 6 row blocks x 5 column tiles, 5 tiles per workgroup on 8
    workgroups; image 1 starts inside row block 2), residual on."""
    from gkgnet_amd import _lib
    lib = _lib.load()
    B, N, C = 2, 324, 320
    R = B * N
    gen = torch.Generator(device="cuda").manual_seed(648)
    w = torch.randn(1, C, C, device="cuda", generator=gen) * 0.1
    dy = torch.randn(R, C, device="cuda", generator=gen)
    res = torch.randn(R, C, device="cuda", generator=gen)
    _, pd = _planes(lib, w, 1, C, C)
    outs = []
    for flags in _three_flags(_lib):
        dx = torch.full((B, C, N), float("nan"), device="cuda")
        dx_tm = torch.full((R, C), float("nan"), device="cuda")
        _lib.check(lib.gkg_linear_dgrad_x6_nchw(dy.data_ptr(), C, pd.data_ptr(), dx.data_ptr(), dx_tm.data_ptr(), R, C, C,
                                                res.data_ptr(), B, N, None, 0, flags, None), "dgrad, channel-major")
        torch.cuda.synchronize()
        assert torch.isnan(dx_tm).all()                                      # the GEMM stored channel-major itself
        outs.append(dx)
    assert torch.isfinite(outs[2]).all() and torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2])
    ref = (dy.double() @ w[0].double() + res.double()).view(B, N, C).transpose(1, 2)
    mag = (dy.double().abs() @ w[0].double().abs() + res.double().abs()).view(B, N, C).transpose(1, 2) + 1e-30
    e = _rel(outs[0], ref, mag)
    f = _rel(torch.addmm(res, dy, w[0]).view(B, N, C).transpose(1, 2), ref, mag)
    print(f"channel-major store: dx {e:.3e} (fp32 {f:.3e})")
    assert e <= max(f, 1.2e-7), (e, f)


@pytest.mark.parametrize("pnb,pact", [(1, 0), (4, 1)])
def test_walk_bn_backward_statistics_epilogue(pnb, pact):
    """gkg_linear_dgrad_x6_bnbwd_sk without a workspace (the tile body), dx (1100, 160) from dy (1100, 320): 9 row blocks x 3 column
    tiles.  This epilogue's walk form measured slower on the MI355X (44.0 -> 47.8 us for cfg2's 810-tile launch) and was taken out
    of the sources, so the three flag sets reach the same launch: the test pins that the entry point accepts them and computes the
    same.  The statistics against the one-tile launch (rtol 1e-12: the same per-tile terms) and against gkg_bn_bwd_stats_f64 on
    the same dx at the bound of tests/test_hip_bwd_stats_in_dgrad.py: max abs difference <= 2e-4 * max(1, max |ref|)."""
    from gkgnet_amd import _lib
    lib = _lib.load()
    R, cin, cout = 1100, 160, 320
    pco = cin // pnb
    gen = torch.Generator(device="cuda").manual_seed(1100 + pnb)
    w = torch.randn(1, cout, cin, device="cuda", generator=gen) / cout ** 0.5
    dy = torch.randn(R, cout, device="cuda", generator=gen)
    Y = torch.randn(pnb, R, pco, device="cuda", generator=gen) * 1.5 + 0.3
    mean = Y.mean(1)
    invstd = 1.0 / torch.sqrt(Y.var(1, unbiased=False) + 1e-5)
    a = (torch.rand(pnb, pco, device="cuda", generator=gen) + 0.5) * invstd
    c = torch.randn(pnb, pco, device="cuda", generator=gen) * 0.3 - mean * a
    mean, invstd, a, c = (t.reshape(-1).contiguous() for t in (mean, invstd, a, c))
    _, pd = _planes(lib, w, 1, cout, cin)
    outs = []
    for flags in _three_flags(_lib):
        dx = torch.full((R, cin), float("nan"), device="cuda")
        sums = torch.zeros(2 * cin, dtype=torch.float64, device="cuda")
        _lib.check(lib.gkg_linear_dgrad_x6_bnbwd_sk(dy.data_ptr(), cout, pd.data_ptr(), dx.data_ptr(), R, cin, cout, None, Y.data_ptr(),
                                                    a.data_ptr(), c.data_ptr(), mean.data_ptr(), invstd.data_ptr(), sums.data_ptr(),
                                                    pnb, pco, pact, None, 0, flags, None), "dgrad + BN backward statistics")
        torch.cuda.synchronize()
        outs.append((dx, sums))
    dx, sums = outs[2]
    assert torch.isfinite(dx).all() and float(sums.abs().max()) > 0
    for dxw, sw in outs[:2]:
        assert torch.equal(dxw, dx)
        torch.testing.assert_close(sw, sums, rtol=1e-12, atol=0.0)
    ref = torch.zeros(2 * cin, dtype=torch.float64, device="cuda")
    _lib.check(lib.gkg_bn_bwd_stats_f64(dx.data_ptr(), Y.data_ptr(), a.data_ptr(), c.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                        R, pco, pnb, cin, pco if pnb > 1 else 0, pact, ref.data_ptr(), None, 0, None), "gkg_bn_bwd_stats_f64")
    torch.cuda.synchronize()
    d = float((outs[0][1] - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    print(f"pnb={pnb} act={pact}: statistics, max abs diff / max(1, max |ref|) = {d:.3e}")
    assert d <= 2e-4
    ref_dx = dy.double() @ w[0].double()
    mag = dy.double().abs() @ w[0].double().abs() + 1e-30
    e, f = _rel(outs[0][0], ref_dx, mag), _rel(dy @ w[0], ref_dx, mag)
    assert e <= max(f, 1.2e-7), (e, f)


def test_the_launch_rule():
    """gkg_x6_walk_workgroups answers with x6_launch's own predicates.  A 6-tile problem (3 row blocks x 2 column tiles) walks on
    8 workgroups when forced with the cap; the same problem with a split-K workspace has its contraction cut across workgroups
    (10 K-steps, 6 tiles) and does not walk; cfg2's shapes: the grouped product (972 tiles, two rounds) walks by itself, fc1 (405,
    one round) does not, and neither does a many-round launch (stage 3's 41 472 x 400 -> 400, 2 268 tiles)."""
    from gkgnet_amd import _lib
    lib = _lib.load()
    forced8 = _lib.X6_FORCE_WALK | (1 << _lib.X6_WALK_CAP_SHIFT)
    assert lib.gkg_x6_walk_workgroups(384, 320, 128, 1, 0, forced8) == 8
    assert lib.gkg_x6_walk_workgroups(384, 320, 128, 1, 0, forced8 | (2 << _lib.X6_WALK_CAP_SHIFT)) == 16     # cap field 3: 2 fit
    assert lib.gkg_x6_walk_workgroups(384, 320, 128, 1, 1, forced8 | _lib.X6_NO_KS) == 0       # split across workgroups
    assert lib.gkg_x6_walk_workgroups(384, 320, 128, 1, 1, forced8) == 0                       # the short-matrix body
    assert lib.gkg_x6_walk_workgroups(384, 320, 128, 1, 0, 0) == 0                             # one round
    assert lib.gkg_x6_walk_workgroups(384, 320, 128, 1, 0, forced8 | _lib.X6_NO_WALK) == 0
    g = lib.gkg_x6_walk_workgroups(10368, 160, 160, 4, 1, 0)
    assert g > 0 and g % 8 == 0 and lib.gkg_x6_walk_workgroups(10368, 160, 160, 4, 1, _lib.X6_NO_WALK) == 0
    assert lib.gkg_x6_walk_workgroups(10368, 320, 320, 1, 1, 0) == 0
    assert lib.gkg_x6_walk_workgroups(41472, 400, 400, 1, 1, 0) == 0 and lib.gkg_x6_walk_workgroups(41472, 400, 400, 1, 1, _lib.X6_FORCE_WALK) > 0
    # and the forced 6-tile launch computes what the one-tile launch computes
    gen = torch.Generator(device="cuda").manual_seed(6)
    x = torch.randn(1, 384, 320, device="cuda", generator=gen)
    w = torch.randn(1, 128, 320, device="cuda", generator=gen) * 0.1
    pf, _ = _planes(lib, w, 1, 128, 320)
    ys = []
    for flags in (forced8, _lib.X6_NO_WALK):
        y = torch.full((1, 384, 128), float("nan"), device="cuda")
        _lib.check(lib.gkg_linear_bn_fwd_x6_sk(x.data_ptr(), 320, 384 * 320, pf.data_ptr(), y.data_ptr(), 384, 320, 128, 1, 0,
                                               *([None] * 10), 0.0, 0.0, None, None, 0, flags, None), "fwd")
        torch.cuda.synchronize()
        ys.append(y)
    assert torch.isfinite(ys[1]).all() and torch.equal(ys[0], ys[1])
