"""The run-independent x6 weight gradients through the C ABI (gkg_linear_wgrad_x6_det / _batch_det, include/gkg_hip.h): fp32
accuracy against fp64, the definition bit for bit — dw = (((0 + P_0) + P_1) + ...) + P_{S-1} over the slabs the library reports —,
identical bits from call to call, and the argument / workspace errors."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

ERR_NULL, ERR_SHAPE, ERR_WORKSPACE = -1, -2, -4
# tests/test_hip_gemm_x6.py::WSHAPES and the six shapes of test_weight_gradient_tile_shapes
WSHAPES = [(10368, 320, 320, 1), (10368, 160, 160, 4), (2560, 1280, 320, 1), (20000, 80, 80, 1), (777, 36, 40, 1),
           (4100, 400, 100, 1), (129, 64, 8, 2), (19, 16, 8, 1), (3000, 1, 3, 1)]
TILE_SHAPES = [(1000, 256, 100, 1), (1000, 320, 256, 1), (2600, 640, 320, 1), (2600, 320, 1280, 1), (777, 128, 128, 3),
               (1000, 320, 320, 1)]
CASE_A, CASE_B, CASE_C, CASE_D = (1024, 40, 72, 1), (3072, 256, 100, 1), (1536, 320, 256, 1), (1408, 24, 40, 4)


def _lib():
    from gkgnet_amd import _lib
    return _lib, _lib.load()


def _i32(t):
    return t.contiguous().view(torch.int32)


def _workspace(lib, R, cin, cout, nb, ldg, ldx, slabs):
    n = lib.gkg_linear_wgrad_x6_det_workspace_bytes(R, cin, cout, nb, ldg, ldx, slabs)
    assert n > 0 and n % 16 == 0
    return torch.empty(n, dtype=torch.uint8, device="cuda")


def _det(dy_ptr, ldg, g_bs, x_ptr, ldx, x_bs, dw, R, cin, cout, nb, kperm=0, slabs=0):
    L, lib = _lib()
    ws = _workspace(lib, R, cin, cout, nb, ldg, ldx, slabs)
    L.check(lib.gkg_linear_wgrad_x6_det(dy_ptr, ldg, g_bs, x_ptr, ldx, x_bs, dw.data_ptr(), R, cin, cout, nb, kperm, slabs,
                                        ws.data_ptr(), ws.numel(), None), "gkg_linear_wgrad_x6_det")
    return dw


def _slabs(R, cin, cout, nb, ldg, ldx, ups, slabs):
    _, lib = _lib()
    first, rows = (ctypes.c_int * 8192)(), (ctypes.c_int * 8192)()
    n = lib.gkg_linear_wgrad_x6_det_slabs(R, cin, cout, nb, ldg, ldx, 1, ups, slabs, first, rows, 8192)
    assert 0 < n <= 8192
    return list(zip(first[:n], rows[:n]))


def _operands(R, cin, cout, nb, seed, sliced=False):
    """(dy, x, ldg, g_bstride, ldx, x_bstride) as (nb, R, c) views: contiguous batches, or (sliced) column slices of (R, nb c)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    if sliced:
        dyw = torch.randn(R, nb * cout, device="cuda", generator=gen)
        xw = torch.randn(R, nb * cin, device="cuda", generator=gen) * 2
        return dyw.view(R, nb, cout).permute(1, 0, 2), xw.view(R, nb, cin).permute(1, 0, 2), nb * cout, cout, nb * cin, cin
    x = torch.randn(nb, R, cin, device="cuda", generator=gen) * 2
    dy = torch.randn(nb, R, cout, device="cuda", generator=gen)
    return dy, x, cout, R * cout, cin, R * cin


def _kperm_cols(t):
    """dw of the operand columns [x chunk | m chunk] -> the reference's interleave: operand column j lands in column 2j / 2(j-ci/2)+1."""
    nb, co, ci = t.shape
    return t.view(nb, co, 2, ci // 2).permute(0, 1, 3, 2).reshape(nb, co, ci)


@pytest.mark.parametrize("R,cin,cout,nb", WSHAPES + TILE_SHAPES)
def test_accuracy_at_the_fp32_bar_into_a_dirty_slot(R, cin, cout, nb):
    dy, x, ldg, gbs, ldx, xbs = _operands(R, cin, cout, nb, R * 3 + cout)
    E, G = nb * cout * cin, 64
    buf = torch.full((E + 2 * G,), float("nan"), device="cuda")
    dw = buf[G:G + E].view(nb, cout, cin)
    dw.fill_(7.0)                                                      # stale contents must not leak
    _det(dy.data_ptr(), ldg, gbs, x.data_ptr(), ldx, xbs, dw, R, cin, cout, nb)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + E:]).all())
    ref = torch.bmm(dy.double().transpose(1, 2), x.double())
    mag = torch.bmm(dy.double().abs().transpose(1, 2), x.double().abs()) + 1e-30
    e = float(((dw.double() - ref).abs() / mag).max())
    f = float(((torch.bmm(dy.transpose(1, 2), x).double() - ref).abs() / mag).max())
    print(f"wgrad_det {R}x{cin}->{cout} nb={nb}: e={e:.3e} fp32={f:.3e}")
    assert e <= max(f, 1.2e-7) and e < 2e-7, (e, f)


def _check_definition(full, partials):
    asc = torch.zeros_like(full)
    for p in partials:
        asc = torch.add(asc, p)
    desc = torch.zeros_like(full)
    for p in reversed(partials):
        desc = torch.add(desc, p)
    torch.cuda.synchronize()
    differ = float((_i32(asc) != _i32(desc)).float().mean())
    print(f"ascending vs descending order: {differ:.3f} of the elements differ")
    assert differ >= 0.2, differ                    # the order is visible in these operands: the equality below says something
    assert torch.equal(_i32(full), _i32(asc))


@pytest.mark.parametrize("shape,slabs,sliced,kperm", [(CASE_A, 8, False, 0), (CASE_B, 12, False, 0), (CASE_C, 4, False, 0),
                                                      (CASE_D, 4, True, 0), (CASE_D, 4, True, 1)])
def test_the_definition_bit_for_bit(shape, slabs, sliced, kperm):
    R, cin, cout, nb = shape
    dy, x, ldg, gbs, ldx, xbs = _operands(R, cin, cout, nb, R + 7 * slabs, sliced)
    plan = _slabs(R, cin, cout, nb, ldg, ldx, 0, slabs)
    assert len(plan) == slabs and sum(r for _, r in plan) == R
    if shape == CASE_D:
        assert [r // 128 for _, r in plan] == [3, 3, 3, 2]
    partials = []
    for first, rows in plan:
        p = torch.full((nb, cout, cin), float("nan"), device="cuda")
        partials.append(_det(dy.data_ptr() + first * ldg * 4, ldg, gbs, x.data_ptr() + first * ldx * 4, ldx, xbs, p, rows, cin, cout,
                             nb, kperm, 1))
    full = _det(dy.data_ptr(), ldg, gbs, x.data_ptr(), ldx, xbs, torch.full((nb, cout, cin), 7.0, device="cuda"), R, cin, cout, nb,
                kperm, slabs)
    _check_definition(full, partials)
    want = torch.bmm(dy.double().transpose(1, 2), x.double())
    if kperm:
        want = _kperm_cols(want)
    assert torch.allclose(full.double(), want, atol=1e-3, rtol=1e-4)


@pytest.mark.parametrize("shape,sliced", [(CASE_A, False), (CASE_D, True), ((1000, 256, 100, 1), False), ((4100, 400, 100, 1), False),
                                          ((129, 64, 8, 2), False)])
def test_five_calls_give_the_same_bits(shape, sliced):
    R, cin, cout, nb = shape
    dy, x, ldg, gbs, ldx, xbs = _operands(R, cin, cout, nb, R + cin, sliced)
    got = []
    for i in range(5):
        dw = torch.full((nb, cout, cin), float(i) - 2.0, device="cuda")
        got.append(_i32(_det(dy.data_ptr(), ldg, gbs, x.data_ptr(), ldx, xbs, dw, R, cin, cout, nb)).clone())
    torch.cuda.synchronize()
    assert all(torch.equal(got[0], g) for g in got[1:])


def test_a_captured_call_replays_the_eager_bits():
    """Every launch of the call is a kernel (no memset node, no host synchronisation): it captures into a hipGraph, and the replay
    overwrites a dirty slot with the bits of the eager call."""
    L, lib = _lib()
    R, cin, cout, nb = 4100, 400, 100, 1                               # main launch + ragged remainder + reduction
    dy, x, ldg, gbs, ldx, xbs = _operands(R, cin, cout, nb, 17)
    ws = _workspace(lib, R, cin, cout, nb, ldg, ldx, 0)
    dw = torch.full((nb, cout, cin), 7.0, device="cuda")

    def call():
        L.check(lib.gkg_linear_wgrad_x6_det(dy.data_ptr(), ldg, gbs, x.data_ptr(), ldx, xbs, dw.data_ptr(), R, cin, cout, nb, 0, 0,
                                            ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "gkg_linear_wgrad_x6_det")
    call()
    torch.cuda.synchronize()
    want = _i32(dw).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for fill in (float("nan"), -3.0):
        dw.fill_(fill)
        ws.fill_(255)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_i32(dw), want)


def _problem(L, dy, x, dw, ldg, gbs, ldx, xbs, R, cin, cout, nb, kperm=0, first=0):
    return L.WgradProblem(dy.data_ptr() + first * ldg * 4, x.data_ptr() + first * ldx * 4, dw.data_ptr(), gbs, xbs, ldg, ldx, R, cin,
                          cout, nb, kperm)


def _batch(problems, ups):
    L, lib = _lib()
    arr = (L.WgradProblem * len(problems))(*problems)
    n = lib.gkg_linear_wgrad_x6_batch_det_workspace_bytes(arr, len(problems), ups)
    assert n > 0 and n % 16 == 0
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    L.check(lib.gkg_linear_wgrad_x6_batch_det(arr, len(problems), ups, ws.data_ptr(), n, None), "gkg_linear_wgrad_x6_batch_det")


@pytest.mark.parametrize("ups", [2, 0])
def test_five_batched_calls_give_the_same_bits(ups):
    L, _ = _lib()
    shapes = [CASE_A + (0,), CASE_C + (0,), (2304, 96, 160, 4, 1), (512, 64, 64, 1, 0)]
    ops = [_operands(R, cin, cout, nb, 11 * i + R) for i, (R, cin, cout, nb, _) in enumerate(shapes)]
    got = []
    for i in range(5):
        dws = [torch.full((nb, cout, cin), float(i) + 0.5, device="cuda") for _, cin, cout, nb, _ in shapes]
        _batch([_problem(L, o[0], o[1], dw, *o[2:], R, cin, cout, nb, kp) for o, dw, (R, cin, cout, nb, kp) in zip(ops, dws, shapes)], ups)
        got.append([_i32(dw).clone() for dw in dws])
    torch.cuda.synchronize()
    for g in got[1:]:
        assert all(torch.equal(a, b) for a, b in zip(got[0], g))
    for o, g, (R, cin, cout, nb, kp) in zip(ops, got[0], shapes):
        want = torch.bmm(o[0].double().transpose(1, 2), o[1].double())
        assert torch.allclose(g.view(torch.float32).view(nb, cout, cin).double(), _kperm_cols(want) if kp else want, atol=1e-3, rtol=1e-4)


def test_the_definition_in_a_one_problem_batch():
    L, _ = _lib()
    R, cin, cout, nb = CASE_A
    dy, x, ldg, gbs, ldx, xbs = _operands(R, cin, cout, nb, 99)
    plan = _slabs(R, cin, cout, nb, ldg, ldx, 2, 0)
    assert len(plan) > 1 and sum(r for _, r in plan) == R
    partials = []
    for first, rows in plan:
        assert len(_slabs(rows, cin, cout, nb, ldg, ldx, 4096, 0)) == 1
        p = torch.full((nb, cout, cin), float("nan"), device="cuda")
        _batch([_problem(L, dy, x, p, ldg, gbs, ldx, xbs, rows, cin, cout, nb, 0, first)], 4096)
        partials.append(p)
    full = torch.full((nb, cout, cin), 7.0, device="cuda")
    _batch([_problem(L, dy, x, full, ldg, gbs, ldx, xbs, R, cin, cout, nb)], 2)
    _check_definition(full, partials)


def test_errors_launch_nothing():
    L, lib = _lib()
    R, cin, cout, nb = CASE_A
    dy, x, ldg, gbs, ldx, xbs = _operands(R, cin, cout, nb, 5)
    dw = torch.full((nb, cout, cin), 7.0, device="cuda")
    need = lib.gkg_linear_wgrad_x6_det_workspace_bytes(R, cin, cout, nb, ldg, ldx, 0)
    ws = torch.full((need + 64,), 3, dtype=torch.uint8, device="cuda")

    def call(R=R, nb=nb, wsp=ws.data_ptr(), nbytes=need):
        return lib.gkg_linear_wgrad_x6_det(dy.data_ptr(), ldg, gbs, x.data_ptr(), ldx, xbs, dw.data_ptr(), R, cin, cout, nb, 0, 0, wsp,
                                           nbytes, None)
    assert call(wsp=None) == ERR_WORKSPACE
    assert call(nbytes=need - 16) == ERR_WORKSPACE
    assert call(wsp=ws.data_ptr() + 4) == ERR_WORKSPACE
    assert call(R=0) == ERR_SHAPE and call(nb=65) == ERR_SHAPE
    p = _problem(L, dy, x, dw, ldg, gbs, ldx, xbs, R, cin, cout, nb)
    arr = (L.WgradProblem * 1)(p)
    bneed = lib.gkg_linear_wgrad_x6_batch_det_workspace_bytes(arr, 1, 0)
    assert 0 < bneed <= need + 64
    assert lib.gkg_linear_wgrad_x6_batch_det(arr, 1, 0, None, bneed, None) == ERR_WORKSPACE
    assert lib.gkg_linear_wgrad_x6_batch_det(arr, 1, 0, ws.data_ptr(), bneed - 16, None) == ERR_WORKSPACE
    assert lib.gkg_linear_wgrad_x6_batch_det(arr, 1, 0, ws.data_ptr() + 4, bneed, None) == ERR_WORKSPACE
    bad = (L.WgradProblem * 2)(p, _problem(L, dy, x, dw, ldg, gbs, ldx, xbs, 0, cin, cout, nb))
    assert lib.gkg_linear_wgrad_x6_batch_det(bad, 2, 0, ws.data_ptr(), need, None) == ERR_SHAPE
    bad = (L.WgradProblem * 2)(p, _problem(L, dy, x, dw, ldg, gbs, ldx, xbs, R, cin, cout, 65))
    assert lib.gkg_linear_wgrad_x6_batch_det(bad, 2, 0, ws.data_ptr(), need, None) == ERR_SHAPE
    assert lib.gkg_linear_wgrad_x6_batch_det(None, 1, 0, ws.data_ptr(), need, None) == ERR_NULL
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((ws == 3).all())            # nothing was launched: slot and workspace keep their fill
    assert call() == 0                                                  # ... and the same call with a good workspace runs
    torch.cuda.synchronize()
    assert not bool((dw == 7.0).any())
