"""Frozen (eval-mode) BatchNorm through the block-level entry points (csrc/gkg_block.hip ``bn_frozen``, gkgnet_amd/block.py) and
the folded affine as the k-NN's token preparation (gkg_affine_knn_prep, reference torch_vertex.py:326 -> torch_edge.py:167-173).

(1) gkg_affine_knn_prep + the k-NN call with GKG_KNN_X_PREPARED / _Y_PREPARED against today's apply kernel (gkg_affine_act,
    gkg_tm_affine_to_nchw_dual) + the same call with its own preparation: identical bits everywhere.
(2) the driver against the per-layer composition on all-frozen Grapher -> GrapherLabel pairs: identical outputs, graphs and input
    gradients, untouched buffers, parameter gradients to the tolerances of tests/test_hip_block_driver.py.
(3) scope: mixed blocks, mode switches under a plan, no_grad.   (4) the prep fusion inside the composition.
(5) descriptor validation of the four entry points (return codes only: nothing is launched)."""
import ctypes

import pytest
import torch

from test_hip_block_driver import SWITCHES, _first_difference

pytestmark = pytest.mark.gpu

SHAPES = [dict(C=64, H=12, L=20, B=48, G=2, d=2), dict(C=80, H=9, L=7, B=5, G=4, d=1)]


def _bits_equal(t0, t1):
    if t0.dtype == torch.float32:
        return torch.equal(t0.view(torch.int32), t1.view(torch.int32))          # (NaN-safe: buffers start NaN-filled)
    return torch.equal(t0, t1)


# ------------------------------------------------------------------------------------------------ (1) the new call
def _modes():
    """Every selection-flag combination _lib.knn_select_flags() can return (GKG_KNN_SELECT / GKG_KNN_PREFILTER)."""
    from gkgnet_amd import _lib
    return {"auto": 0, "buffered": _lib.KNN_SELECT_BUFFERED | _lib.KNN_NO_PREFILTER, "direct": _lib.KNN_SELECT_DIRECT | _lib.KNN_NO_PREFILTER,
            "no_prefilter": _lib.KNN_NO_PREFILTER, "prefilter": _lib.KNN_FORCE_PREFILTER}


def _poisoned_ws(nbytes):
    return torch.full((nbytes,), 255, dtype=torch.uint8, device="cuda")           # all-ones bytes: NaN wherever nothing was written


def _compare_queries(lib, B, G, c, N, M, k, d, relpos, sel, seed):
    """fc1's form: out = a y + c into the x half of an XM buffer (ochunk = C / 4, ldo = 2 C); self graph (M None) or label graph."""
    from gkgnet_amd import _lib
    C = G * c
    Mk = N if M is None else M
    g = torch.Generator(device="cuda").manual_seed(seed)
    Y = torch.randn(B * N, C, device="cuda", generator=g) * 1.7 + 0.3
    a = torch.rand(C, device="cuda", generator=g) + 0.5
    cs = torch.randn(C, device="cuda", generator=g) * 0.3
    y = None if M is None else torch.randn(B, Mk, C, device="cuda", generator=g)
    rp = (-torch.rand(N, Mk, device="cuda", generator=g)) if relpos else None
    flags = _lib.KNN_NORMALIZE | sel | (_lib.KNN_RELPOS_UNIT if relpos else 0)
    has_y, has_rp = (0 if y is None else 1), (1 if relpos else 0)
    yp, rpp = (None if y is None else y.data_ptr()), (None if rp is None else rp.data_ptr())
    wsb = lib.gkg_knn_workspace_bytes(B * G, c, N, Mk, k, d, _lib.F32, _lib.KNN_NORMALIZE)
    forms = [0] + ([1] if lib.gkg_knn_mr_fused_supported(B, G, c, N, Mk, k, d, has_y, has_rp, flags) == 1 else [])
    for fm in forms:
        def run(prep):
            XM = torch.full((B * N, 2 * C), float("nan"), device="cuda")
            ws = _poisoned_ws(wsb)
            f = flags
            if prep:
                _lib.check(lib.gkg_affine_knn_prep(Y.data_ptr(), a.data_ptr(), cs.data_ptr(), XM.data_ptr(), 2 * C, C // 4, B, G, c, N, Mk,
                                                   k, d, has_y, has_rp, flags, fm, 0, None, None, ws.data_ptr(), wsb, None),
                           "gkg_affine_knn_prep")
                f |= _lib.KNN_X_PREPARED
            else:
                _lib.check(lib.gkg_affine_act(Y.data_ptr(), a.data_ptr(), cs.data_ptr(), None, XM.data_ptr(), B * N, C, 1, 2 * C, 0,
                                              C // 4, 0, _lib.F32, None, 0, None), "gkg_affine_act")
            x_half = XM.clone()
            arg = torch.zeros((B, N, C), dtype=torch.int16, device="cuda")
            nn16 = torch.zeros((B * G, N, k), dtype=torch.int16, device="cuda")
            if fm:
                _lib.check(lib.gkg_knn_mr_fwd_tm(XM.data_ptr(), 2 * C, C // 4, yp, rpp, XM.data_ptr(), arg.data_ptr(), nn16.data_ptr(), None,
                                                 None, B, G, c, N, Mk, k, d, f, ws.data_ptr(), wsb, None), "gkg_knn_mr_fwd_tm")
            else:
                _lib.check(lib.gkg_knn_fwd_tm16(XM.data_ptr(), 2 * C, C // 4, yp, rpp, nn16.data_ptr(), B, G, c, N, Mk, k, d, _lib.F32, f,
                                                ws.data_ptr(), wsb, None), "gkg_knn_fwd_tm16")
                _lib.check(lib.gkg_mr_fwd_tm16(XM.data_ptr(), 2 * C, C // 4, yp, nn16.data_ptr(), XM.data_ptr(), arg.data_ptr(), B, G, c, N,
                                               Mk, k, 1, _lib.F32, 1, None), "gkg_mr_fwd_tm16")
            torch.cuda.synchronize()
            return dict(out=x_half, XM=XM, arg=arg, nn16=nn16)
        r0, r1 = run(False), run(True)
        assert not torch.isnan(r0["XM"]).any()
        for key in r0:
            assert _bits_equal(r0[key], r1[key]), (key, fm, B, G, c, N, M, relpos, sel)


def _compare_keys(lib, B, G, c, L, M, k, d, relpos, sel, seed):
    """A Grapher's last layer as the producer of the label graph's keys: a y + c + res_tm token-major and channel-major."""
    from gkgnet_amd import _lib
    C = G * c
    g = torch.Generator(device="cuda").manual_seed(seed)
    Y = torch.randn(B * M, C, device="cuda", generator=g) * 1.7 + 0.3
    a = torch.rand(C, device="cuda", generator=g) + 0.5
    cs = torch.randn(C, device="cuda", generator=g) * 0.3
    res = torch.randn(B * M, C, device="cuda", generator=g)
    xq = torch.randn(B, L, C, device="cuda", generator=g)
    rp = (-torch.rand(L, M, device="cuda", generator=g)) if relpos else None
    rpp, has_rp = (None if rp is None else rp.data_ptr()), (1 if relpos else 0)
    flags = _lib.KNN_NORMALIZE | sel | (_lib.KNN_RELPOS_UNIT if relpos else 0)
    wsb = lib.gkg_knn_workspace_bytes(B * G, c, L, M, k, d, _lib.F32, _lib.KNN_NORMALIZE)
    forms = [0] + ([1] if lib.gkg_knn_mr_fused_supported(B, G, c, L, M, k, d, 1, has_rp, flags) == 1 else [])
    for fm in forms:
        def run(prep):
            nchw = torch.full((B, C, M), float("nan"), device="cuda")
            tm = torch.full((B * M, C), float("nan"), device="cuda")
            ws = _poisoned_ws(wsb)
            f = flags
            if prep:
                _lib.check(lib.gkg_affine_knn_prep(Y.data_ptr(), a.data_ptr(), cs.data_ptr(), tm.data_ptr(), 0, 0, B, G, c, L, M, k, d, 1,
                                                   has_rp, flags, fm, 1, res.data_ptr(), nchw.data_ptr(), ws.data_ptr(), wsb, None),
                           "gkg_affine_knn_prep (keys)")
                f |= _lib.KNN_Y_PREPARED
            else:
                _lib.check(lib.gkg_tm_affine_to_nchw_dual(Y.data_ptr(), a.data_ptr(), cs.data_ptr(), res.data_ptr(), nchw.data_ptr(),
                                                          tm.data_ptr(), B, C, M, None), "gkg_tm_affine_to_nchw_dual")
            XM = torch.full((B * L, 2 * C), float("nan"), device="cuda")
            arg = torch.zeros((B, L, C), dtype=torch.int16, device="cuda")
            nn16 = torch.zeros((B * G, L, k), dtype=torch.int16, device="cuda")
            if fm:
                _lib.check(lib.gkg_knn_mr_fwd_tm(xq.data_ptr(), 0, 0, tm.data_ptr(), rpp, XM.data_ptr(), arg.data_ptr(), nn16.data_ptr(), None,
                                                 None, B, G, c, L, M, k, d, f, ws.data_ptr(), wsb, None), "gkg_knn_mr_fwd_tm")
            else:
                _lib.check(lib.gkg_knn_fwd_tm16(xq.data_ptr(), 0, 0, tm.data_ptr(), rpp, nn16.data_ptr(), B, G, c, L, M, k, d, _lib.F32, f,
                                                ws.data_ptr(), wsb, None), "gkg_knn_fwd_tm16")
                _lib.check(lib.gkg_mr_fwd_tm16(xq.data_ptr(), 0, 0, tm.data_ptr(), nn16.data_ptr(), XM.data_ptr(), arg.data_ptr(), B, G, c, L,
                                               M, k, 1, _lib.F32, 1, None), "gkg_mr_fwd_tm16")
            torch.cuda.synchronize()
            return dict(out=tm, out_nchw=nchw, XM=XM, arg=arg, nn16=nn16)
        r0, r1 = run(False), run(True)
        assert not torch.isnan(r0["out"]).any() and not torch.isnan(r0["out_nchw"]).any()
        for key in r0:
            assert _bits_equal(r0[key], r1[key]), (key, fm, B, G, c, L, M, relpos, sel)


@pytest.mark.parametrize("c", [4, 20, 36])
@pytest.mark.parametrize("form", ["queries_self", "queries_label", "keys"])
def test_affine_knn_prep_matches_apply_plus_own_preparation(form, c):
    """Small shapes (cooperative preparation kernel; with the prefilter forced, c >= 16: thread-per-token + the bf16 hi / lo
    planes), ragged tiles (N = 50, 129), every selection mode, relative position on and off."""
    from gkgnet_amd import _lib
    lib = _lib.load()
    B, G, k, d = 2, 4, 5, 2
    for N in (50, 129):
        for relpos in (False, True):
            for name, sel in _modes().items():
                seed = 1000 * c + 10 * N + relpos
                if form == "queries_self":
                    _compare_queries(lib, B, G, c, N, None, k, d, relpos, sel, seed)
                elif form == "queries_label":
                    _compare_queries(lib, B, G, c, N, 60, k, d, relpos, sel, seed)
                else:
                    _compare_keys(lib, B, G, c, 7, N, k, d, relpos, sel, seed)


@pytest.mark.parametrize("form", ["queries_self", "keys"])
def test_affine_knn_prep_on_the_thread_per_token_side(form):
    """The dispatcher (launch_prep) takes the cooperative kernel up to 262 144 token-groups and one thread per token above:
    16 * 4 * 4100 = 262 400 (Y is 4.2 MB).  The shapes of the test above lie on the cooperative side."""
    from gkgnet_amd import _lib
    lib = _lib.load()
    B, G, c, N = 16, 4, 4, 4100
    assert B * G * N > 262144
    if form == "queries_self":
        _compare_queries(lib, B, G, c, N, None, 5, 2, False, 0, 5)
    else:
        _compare_keys(lib, B, G, c, 7, N, 5, 2, False, 0, 6)


# ------------------------------------------------------------------------------------------------ (2) driver vs composition
def _bns(*mods):
    return [m for mod in mods for m in mod.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


def _pair(variant, monkeypatch, C, H, L, G, d):
    """Grapher -> GrapherLabel with conv biases, every BatchNorm frozen the way ``variant`` says; running statistics and affine
    parameters away from their initial values."""
    from gkgnet_amd import layers
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    if variant == "sync":
        monkeypatch.setitem(layers.norm_cfg, "type", "BN")              # plain BatchNorm2d, converted below
    torch.manual_seed(11)
    g = Grapher(C, 9, d, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=True, use_multi_group=True, num_group=G)
    gl = GrapherLabel(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=False, num_nodes=L,
                      use_multi_group=True, num_group=G)
    with torch.no_grad():
        for m in _bns(g, gl):
            m.weight.uniform_(0.5, 1.5)
            m.bias.normal_(0.0, 0.1)
            m.running_mean.normal_(0.0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    if variant == "sync":
        g, gl = torch.nn.SyncBatchNorm.convert_sync_batchnorm(g), torch.nn.SyncBatchNorm.convert_sync_batchnorm(gl)
        assert all(type(m) is torch.nn.SyncBatchNorm for m in _bns(g, gl))
    g, gl = g.cuda(), gl.cuda()
    if variant == "eval":
        g.eval(), gl.eval()
    else:
        layers.freeze_batchnorm(g, affine=(variant == "frozen_affine")).train()
        layers.freeze_batchnorm(gl, affine=(variant == "frozen_affine")).train()
    assert all(not m.training for m in _bns(g, gl))
    assert all(m[0].bias is not None for m in (g.fc1, g.fc2, g.graph_conv.gconv.nn, gl.fc1, gl.fc2, gl.ffn.fc1, gl.ffn.fc2))
    return g, gl


def _count_driver(block, monkeypatch):
    calls = {"g": 0, "l": 0}
    rg, rl = block._GrapherBlockFn.forward, block._LabelBlockFn.forward
    monkeypatch.setattr(block._GrapherBlockFn, "forward", staticmethod(lambda *a: (calls.__setitem__("g", calls["g"] + 1), rg(*a))[1]))
    monkeypatch.setattr(block._LabelBlockFn, "forward", staticmethod(lambda *a: (calls.__setitem__("l", calls["l"] + 1), rl(*a))[1]))

    def restore():
        monkeypatch.setattr(block._GrapherBlockFn, "forward", staticmethod(rg))
        monkeypatch.setattr(block._LabelBlockFn, "forward", staticmethod(rl))
    return calls, restore


def _steps(g, gl, B, C, H, L, bucket, nsteps=3):
    from gkgnet_amd import parallel
    params = list(g.parameters()) + list(gl.parameters())
    names = [n for n, _ in list(g.named_parameters()) + list(gl.named_parameters())]
    bk = parallel.GradBucket(params) if bucket else None
    gen = torch.Generator(device="cuda").manual_seed(3)
    steps = []
    for step in range(nsteps):
        x = torch.randn(B, C, H, H, device="cuda", generator=gen).requires_grad_(True)
        e = torch.randn(B, L, C, device="cuda", generator=gen).requires_grad_(True)
        cx, ce = torch.randn(B, C, H, H, device="cuda", generator=gen), torch.randn(B, L, C, device="cuda", generator=gen)
        if bk is not None:
            bk.release(prezero=True)
        else:
            for p in params:
                p.grad = None
        out = g(x)
        e2, edge = gl(e, out)
        torch.autograd.backward([out, e2], [cx, ce])
        if bk is not None:
            bk.pack()
        torch.cuda.synchronize()
        steps.append(dict(out=out.detach().clone(), e2=e2.detach().clone(), edge=edge.clone(), dx=x.grad.clone(), de=e.grad.clone(),
                          grads=[None if p.grad is None else p.grad.clone() for p in params],
                          bufs=[b.clone() for b in list(g.buffers()) + list(gl.buffers())], names=names,
                          frozen=[not p.requires_grad for p in params]))
    return steps


def _run(driver, variant, monkeypatch, C, H, L, B, G, d, bucket):
    from gkgnet_amd import block
    monkeypatch.setattr(block, "ENABLED", driver)
    g, gl = _pair(variant, monkeypatch, C, H, L, G, d)
    before = [b.clone() for b in list(g.buffers()) + list(gl.buffers())]
    calls, restore = _count_driver(block, monkeypatch)
    try:
        steps = _steps(g, gl, B, C, H, L, bucket)
    finally:
        restore()
    return calls, steps, before


@pytest.mark.parametrize("bucket", [False, True])
@pytest.mark.parametrize("variant", ["frozen", "frozen_affine", "eval", "sync"])
@pytest.mark.parametrize("shape", SHAPES)
def test_frozen_blocks_through_the_driver_match_the_composition(shape, variant, bucket, monkeypatch):
    """Three steps (the dual layout engages at step 2, the prepared label keys at step 3).  Frozen mode has no run-dependent
    statistic in the forward or the input gradients: no retry, bit equality at once."""
    c1, on, before = _run(True, variant, monkeypatch, bucket=bucket, **shape)
    c0, off, _ = _run(False, variant, monkeypatch, bucket=bucket, **shape)
    assert c1 == {"g": 3, "l": 3} and c0 == {"g": 0, "l": 0}, (c1, c0)
    assert _first_difference(on, off) is None, _first_difference(on, off)
    for steps in (on, off):
        for s in steps:
            assert all(torch.equal(u, v) for u, v in zip(s["bufs"], before)), "a frozen BN buffer changed"
            for name, gr, fz in zip(s["names"], s["grads"], s["frozen"]):
                assert (gr is None) == fz, name            # every trainable parameter (conv biases included) got a gradient, no other
    # (the Grapher's relative_pos is never trained; affine=False freezes the 2 x 8 BN scales and shifts as well)
    assert sum(on[0]["frozen"]) == (1 + 16 if variant in ("frozen", "sync") else 1)


@pytest.mark.parametrize("switch", SWITCHES)
def test_frozen_blocks_through_the_driver_match_the_composition_with_a_switch_off(switch, monkeypatch):
    """The frozen form of the driver's other branches (test_hip_block_driver.py: un-prepared queries, the two-launch graph, the
    un-fused backward tail; DGRAD_STATS has nothing to switch in a frozen block and must change nothing): bit equality at once."""
    from gkgnet_amd import fused
    monkeypatch.setattr(fused, switch, False)
    c1, on, _ = _run(True, "frozen_affine", monkeypatch, bucket=False, **SHAPES[1])
    c0, off, _ = _run(False, "frozen_affine", monkeypatch, bucket=False, **SHAPES[1])
    assert c1 == {"g": 3, "l": 3} and c0 == {"g": 0, "l": 0}, (c1, c0)
    assert _first_difference(on, off) is None, _first_difference(on, off)


# ------------------------------------------------------------------------------------------------ (3) scope
def test_a_mixed_block_keeps_the_composition(monkeypatch):
    """fc1's BN in train mode, the rest frozen: the flag is per block, so both blocks are composed layer by layer.  The train-mode
    layer's batch statistics come from fp64 atomics (a mean on an fp32 rounding tie is run-dependent, tests/test_hip_block_driver.py):
    a pair of runs that differs is repeated, as there."""
    from gkgnet_amd import block
    shape = SHAPES[1]
    diff = None
    for attempt in range(4):
        res = {}
        for driver in (True, False):
            monkeypatch.setattr(block, "ENABLED", driver)
            g, gl = _pair("eval", monkeypatch, shape["C"], shape["H"], shape["L"], shape["G"], shape["d"])
            g.fc1[1].train()
            gl.fc1[1].train()
            calls, restore = _count_driver(block, monkeypatch)
            try:
                res[driver] = _steps(g, gl, shape["B"], shape["C"], shape["H"], shape["L"], False, nsteps=2)
            finally:
                restore()
            assert calls == {"g": 0, "l": 0}, (driver, calls)
        diff = _first_difference(res[True], res[False])
        if diff is None:
            return
    raise AssertionError(diff)


def test_a_mode_switch_drops_the_plan(monkeypatch):
    from gkgnet_amd import block
    monkeypatch.setattr(block, "ENABLED", True)
    g, gl = _pair("eval", monkeypatch, 64, 12, 20, 2, 1)
    x = torch.randn(4, 64, 12, 12, device="cuda")
    e = torch.randn(4, 20, 64, device="cuda")
    out = g(x)
    gl(e, out)
    assert block.try_grapher(g, x) is not None and block.try_label(gl, e, out) is not None          # the frozen plans answer
    # frozen -> train: one BN, then the whole module
    g.fc2[1].train()
    gl.ffn.fc1[1].train()
    assert block.try_grapher(g, x) is None and block.try_label(gl, e, out) is None
    gl(e, g(x))                                                                                       # mixed: the composition, no plan
    assert block.try_grapher(g, x) is None and block.try_label(gl, e, out) is None
    g.train(), gl.train()
    assert block.try_grapher(g, x) is None and block.try_label(gl, e, out) is None                  # the recorded mode was frozen
    out = g(x)
    gl(e, out)
    assert block.try_grapher(g, x) is not None and block.try_label(gl, e, out) is not None          # ... a train-mode plan now
    # train -> frozen
    g.fc1[1].eval()
    gl.fc1[1].eval()
    assert block.try_grapher(g, x) is None and block.try_label(gl, e, out) is None
    g.eval(), gl.eval()
    assert block.try_grapher(g, x) is None and block.try_label(gl, e, out) is None
    out = g(x)
    gl(e, out)
    assert block.try_grapher(g, x) is not None and block.try_label(gl, e, out) is not None


def test_eval_without_gradients_keeps_the_composition(monkeypatch):
    from gkgnet_amd import block
    monkeypatch.setattr(block, "ENABLED", True)
    g, gl = _pair("eval", monkeypatch, 64, 12, 20, 2, 1)
    x = torch.randn(4, 64, 12, 12, device="cuda")
    e = torch.randn(4, 20, 64, device="cuda")
    calls, restore = _count_driver(block, monkeypatch)
    try:
        with torch.no_grad():
            for _ in range(2):
                gl(e, g(x))
    finally:
        restore()
    assert calls == {"g": 0, "l": 0}


# ------------------------------------------------------------------------------------------------ (4) prep fusion in the composition
@pytest.mark.parametrize("deterministic", [False, True])
def test_frozen_composition_prepares_the_tokens_in_the_apply_pass(deterministic, monkeypatch):
    """block.ENABLED off, fused.KNN_PREP on / off: same bits, and with it on every block's fc1 (and, once the label block has told
    the Grapher which graph it builds, the Grapher's last layer) goes through gkg_affine_knn_prep.  The switch only changes forward
    launches, so under GKG_DETERMINISTIC (no atomics in the weight / BN-parameter gradients) EVERYTHING is torch.equal; in the
    default mode the outputs, the graph and the input gradients are, and the atomically accumulated parameter gradients agree to
    the tolerances of tests/test_hip_block_driver.py."""
    from gkgnet_amd import _lib, block, fused
    lib = _lib.load()
    monkeypatch.setattr(block, "ENABLED", False)
    monkeypatch.setattr(fused, "DETERMINISTIC", deterministic)
    shape = SHAPES[0]
    real = lib.gkg_affine_knn_prep
    res, count = {}, {}
    for prep in (True, False):
        monkeypatch.setattr(fused, "KNN_PREP", prep)
        n = [0]

        def counted(*a, _n=n):
            _n[0] += 1
            return real(*a)
        monkeypatch.setattr(lib, "gkg_affine_knn_prep", counted)
        try:
            g, gl = _pair("frozen_affine", monkeypatch, shape["C"], shape["H"], shape["L"], shape["G"], shape["d"])
            res[prep] = _steps(g, gl, shape["B"], shape["C"], shape["H"], shape["L"], False, nsteps=3)
        finally:
            monkeypatch.setattr(lib, "gkg_affine_knn_prep", real)
        count[prep] = n[0]
    assert count[False] == 0 and count[True] >= 2 * 3, count              # at least one per block and step
    assert _first_difference(res[True], res[False]) is None, _first_difference(res[True], res[False])
    if deterministic:
        for a, b in zip(res[True], res[False]):
            for name, u, v in zip(a["names"], a["grads"], b["grads"]):
                assert (u is None and v is None) or torch.equal(u, v), name


# ------------------------------------------------------------------------------------------------ (5) descriptor validation
def _fill(obj, ptr, skip=()):
    """Every pointer field of a descriptor (sub-structures included) -> ``ptr``; sizes stay zero."""
    for name, tp in obj._fields_:
        if name in skip:
            continue
        if tp is ctypes.c_void_p:
            setattr(obj, name, ptr)
        elif issubclass(tp, ctypes.Structure):
            _fill(getattr(obj, name), ptr)


def _proj(p, cin, cout, nb, frozen):
    p.cin, p.cout, p.nb, p.eps, p.momentum = cin, cout, nb, 1e-5, 0.1
    if not frozen:
        p.dbias = None                                   # (a conv bias's gradient belongs to the frozen form)


@pytest.mark.parametrize("frozen", [0, 1])
def test_entry_points_validate_the_descriptor_before_any_launch(frozen):
    """graph.G == 0 -> GKG_ERR_SHAPE (it used to be a host division by zero), keys_G == 0 with keys_ws set likewise, a null saved
    activation in the backward -> GKG_ERR_NULL.  Return codes only: each call returns from the shared validation helper, which runs
    before the first launch (every pointer is a live 4 KB buffer all the same)."""
    from gkgnet_amd import _lib, block
    lib = _lib.load()
    ERR_NULL, ERR_SHAPE = -1, -2
    live = torch.zeros(1024, device="cuda")
    C = 64

    def grapher():
        d = block.GrapherBlock()
        _fill(d, live.data_ptr(), skip=("keys_ws",))
        d.B, d.C, d.H, d.W, d.bn_frozen = 1, C, 2, 2, frozen
        _proj(d.fc1, C, C, 1, frozen), _proj(d.conv, C // 2, C // 2, 4, frozen), _proj(d.fc2, 2 * C, C, 1, frozen)
        d.graph.G, d.graph.k, d.graph.d = 2, 2, 1
        return d

    def label():
        d = block.LabelBlock()
        _fill(d, live.data_ptr())
        d.B, d.C, d.L, d.M, d.bn_frozen = 1, C, 2, 4, frozen
        _proj(d.fc1, C, C, 1, frozen), _proj(d.conv, C // 2, C // 2, 4, frozen), _proj(d.fc2, 2 * C, C, 1, frozen), _proj(d.ffn1, C, 2 * C, 1, frozen), _proj(d.ffn2, 2 * C, C, 1, frozen)
        d.graph.G, d.graph.k, d.graph.d = 2, 2, 1
        return d
    wq = (_lib.WgradProblem * 5)()
    calls = {"gkg_grapher_fwd": lambda d: lib.gkg_grapher_fwd(ctypes.byref(d), None),
             "gkg_grapher_bwd": lambda d: lib.gkg_grapher_bwd(ctypes.byref(d), wq, None),
             "gkg_grapher_label_fwd": lambda d: lib.gkg_grapher_label_fwd(ctypes.byref(d), None),
             "gkg_grapher_label_bwd": lambda d: lib.gkg_grapher_label_bwd(ctypes.byref(d), wq, None)}
    for name, call in calls.items():
        make = label if "label" in name else grapher
        d = make()
        d.graph.G = 0
        assert call(d) == ERR_SHAPE, name
        d = make()
        d.graph.G = 3                                    # C % G != 0
        assert call(d) == ERR_SHAPE, name
        if name.endswith("_bwd"):
            for field in ("XM", "A2"):
                d = make()
                setattr(d, field, None)
                assert call(d) == ERR_NULL, (name, field)
            d = make()
            d.fc2.Y = None
            assert call(d) == ERR_NULL, (name, "fc2.Y")
            d = make()
            d.fc1.planes_dgrad = None
            assert call(d) == ERR_NULL, (name, "fc1.planes_dgrad")
    d = grapher()
    d.keys_ws, d.keys_G = live.data_ptr(), 0
    assert lib.gkg_grapher_fwd(ctypes.byref(d), None) == ERR_SHAPE
    torch.cuda.synchronize()
