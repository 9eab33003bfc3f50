"""Training through frozen (eval-mode) BatchNorm on the fused HIP path: the F22 fixture (the reference's Grapher -> GrapherLabel
chain, modules in train(), every BatchNorm in eval()), whole-module eval() with gradients, the gkg_bn_eval_bwd kernel on its
own, determinism, mixed train / frozen layers, DropPath, bf16 autocast and a tiny backbone with ``norm_eval=True``."""
import math

import numpy as np
import pytest
import torch
from torch.nn.modules.batchnorm import _BatchNorm

from util import check_indices, load_fixture, state_from

pytestmark = pytest.mark.gpu
TOL = dict(atol=1e-3, rtol=1e-3)          # the project's module tolerance (test_hip_modules.py)
PTOL = dict(atol=2e-3, rtol=2e-3)         # parameter gradients (test_hip_modules._check_param_grads)


def _t(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bns(*mods):
    return [m for mod in mods for m in mod.modules() if isinstance(m, _BatchNorm)]


def _buffers(*mods):
    return [b.detach().clone() for m in _bns(*mods) for b in (m.running_mean, m.running_var, m.num_batches_tracked)]


@pytest.fixture(params=["fused", "composable"])
def path(request):
    from gkgnet_amd import fused
    old = fused.ENABLED
    fused.ENABLED = request.param == "fused"
    yield request.param
    fused.ENABLED = old


def _modules(meta, a, drop_path=0.0):
    """The F22 pair with the fixture's weights, modules in train(), every BatchNorm in eval()."""
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    C, k, d, G, n, L = meta["C"], meta["k"], meta["dilation"], meta["G"], meta["n"], meta["L"]
    g = Grapher(C, k, d, "mr", "gelu", "batch", True, False, 0.2, 1, n=n, drop_path=drop_path, relative_pos=True,
                use_multi_group=True, num_group=G)
    gl = GrapherLabel(C, k, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=n, drop_path=drop_path, relative_pos=False,
                      num_nodes=L, use_multi_group=True, num_group=G)
    res = g.load_state_dict(state_from(a, "g/sd/"), strict=False)      # relative_pos is not stored: a function of (C, n) alone
    assert res.missing_keys == ["relative_pos"] and not res.unexpected_keys
    gl.load_state_dict(state_from(a, "gl/sd/"))
    g.cuda().train()
    gl.cuda().train()
    for m in _bns(g, gl):
        m.eval()
    return g, gl


class _Spy:
    """Counts the calls of the fused entry points and keeps the Grapher's graph (the fused Grapher discards it otherwise)."""

    def __init__(self, g):
        from gkgnet_amd import fused
        self.fused, self.calls, self.label_calls, self.edge = fused, 0, 0, None
        self.real, self.real_label = fused.grapher_forward, fused.grapher_label_forward
        self.hook = g.graph_conv.register_forward_hook(lambda m, i, o: setattr(self, "edge", o[1].detach()))

    def __enter__(self):
        def spy(*args, **kw):
            kw["want_edge"] = True
            out = self.real(*args, **kw)
            self.calls += 1
            self.edge = out[1].detach()
            return out

        def spy_label(*args, **kw):
            self.label_calls += 1
            return self.real_label(*args, **kw)
        self.fused.grapher_forward, self.fused.grapher_label_forward = spy, spy_label
        return self

    def __exit__(self, *exc):
        self.fused.grapher_forward, self.fused.grapher_label_forward = self.real, self.real_label
        self.hook.remove()


def _step(g, gl, a, x_grad=True):
    x, e = _t(a["x"]).requires_grad_(x_grad), _t(a["e"]).requires_grad_(x_grad)
    out = g(x)
    e2, idx = gl(e, out)
    ((out * _t(a["cot_out"])).sum() + (e2 * _t(a["cot_e"])).sum()).backward()
    return out.detach(), e2.detach(), idx.detach(), x.grad, e.grad


def _check_values(meta, a, out, e2, idx, dx, de, edge):
    assert check_indices(edge[0].cpu().numpy(), a["edge_index"][0], a["topd"], a["topi"], meta["dilation"]) == 0
    assert np.array_equal(edge[1].cpu().numpy(), a["edge_index"][1])
    assert idx.shape == a["nn_idx"].shape
    assert check_indices(idx.cpu().numpy(), a["nn_idx"], a["label_topd"], a["label_topi"]) == 0
    for name, got, want in (("out", out, "out"), ("e2", e2, "e2"), ("dx", dx, "dx"), ("de", de, "de")):
        err = float((got - _t(a[want])).abs().max())
        print(f"{name}: max |err| {err:.3e} (scale {float(np.abs(a[want]).max()):.3e})")
        assert torch.allclose(got, _t(a[want]), **TOL), (name, err)


def _check_param_grads(a, g, gl):
    for prefix, mod in (("g/", g), ("gl/", gl)):
        named = dict(mod.named_parameters())
        want = state_from(a, prefix + "grad/")
        assert set(want) == {k for k, p in named.items() if p.requires_grad}
        for k, w in want.items():
            got = named[k].grad
            assert got is not None, f"{prefix}{k}: no gradient (a conv bias in front of an eval-mode BN has a real one)"
            err = float((got - w.cuda()).abs().max())
            assert torch.allclose(got, w.cuda(), **PTOL), (prefix + k, err)


# ------------------------------------------------------------------------------------------------ (1) the idiom
def test_frozen_bn_step_matches_reference(path):
    """modules.train() + every BatchNorm in eval(): forward, graphs, input gradients and EVERY parameter gradient (conv biases
    included) against the reference's own numbers, on the fused path (which must actually run) and on the composable one."""
    meta, a = load_fixture("f22_frozen_bn")
    g, gl = _modules(meta, a)
    before = _buffers(g, gl)
    with _Spy(g) as spy:
        out, e2, idx, dx, de = _step(g, gl, a)
    if path == "fused":
        assert spy.calls >= 1 and spy.label_calls >= 1, "the fused token-major path was expected to run"
    else:
        assert spy.calls == 0 and spy.label_calls == 0
    _check_values(meta, a, out, e2, idx, dx, de, spy.edge)
    _check_param_grads(a, g, gl)
    assert all(torch.equal(x, y) for x, y in zip(before, _buffers(g, gl)))


# ------------------------------------------------------------------------------------------------ (2) whole-module eval()
@pytest.mark.parametrize("trainable", [False, True])
def test_whole_module_eval_with_gradients(trainable):
    """Modules in eval() with gradients enabled (Grad-CAM / adversarial evaluation; fine-tuning with everything frozen):
    the fused path is taken and gives the fixture's values — input gradients only, or with trainable parameters."""
    meta, a = load_fixture("f22_frozen_bn")
    g, gl = _modules(meta, a)
    g.eval()
    gl.eval()
    for p in list(g.parameters()) + list(gl.parameters()):
        if p.dtype.is_floating_point and p is not getattr(g, "relative_pos", None):
            p.requires_grad_(trainable)
    with _Spy(g) as spy:
        out, e2, idx, dx, de = _step(g, gl, a)
    assert spy.calls >= 1 and spy.label_calls >= 1, "eval() with gradients must take the fused path"
    _check_values(meta, a, out, e2, idx, dx, de, spy.edge)
    if trainable:
        _check_param_grads(a, g, gl)
    else:
        assert all(p.grad is None for p in list(g.parameters()) + list(gl.parameters()))


# ------------------------------------------------------------------------------------------------ (3) statistics untouched
def test_running_statistics_are_bit_identical_after_two_steps():
    meta, a = load_fixture("f22_frozen_bn")
    g, gl = _modules(meta, a)
    before = _buffers(g, gl)
    for _ in range(2):
        _step(g, gl, a)
    torch.cuda.synchronize()
    after = _buffers(g, gl)
    assert len(before) == len(after) == 3 * 8
    assert all(torch.equal(x, y) for x, y in zip(before, after))


# ------------------------------------------------------------------------------------------------ (4) the kernel
def _gelu_grad64(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("scaled", [False, True])
def test_bn_eval_bwd_kernel(nb, act, scaled):
    """gkg_bn_eval_bwd through ctypes: strided dout, C not a multiple of 64, R not a multiple of the row tile.
    dY against the fp64 formula (the tolerances of test_hip_dense.py::test_linear_bn_act_matches_torch for an input gradient);
    dbeta / dgamma / dbias against fp64 sums of the kernel's OWN dY / a, which isolates the accumulation: fp64 accumulation of
    fp32 products must agree to 1e-6 * sum |term| per column (three fp32 roundings per term give <= 3 * 2^-24 ~ 1.8e-7; the rest
    is room for the division in the check itself); the NULL-sums form gives the same dY bit for bit; the deterministic
    (workspace) form gives the same dY, sums within the same bound, and identical bits on a second run."""
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    lib = _lib.load()
    R, C, rps, eps = 777, 72, 100, 1e-5
    gen = torch.Generator(device="cuda").manual_seed(100 * nb + 10 * act + int(scaled))
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    ldg = nb * C + 8
    bstride = C if nb > 1 else 0
    dout_full = rnd(R, ldg)
    Y = (rnd(nb, R, C) * 1.5 + 0.3).contiguous()
    gamma = (torch.rand(nb * C, device="cuda", generator=gen) + 0.5) * torch.where(rnd(nb * C) > 0, 1.0, -1.0)
    beta, bias, rm = rnd(nb * C) * 0.3, rnd(nb * C) * 0.3, rnd(nb * C) * 0.3 + 0.3
    rv = torch.rand(nb * C, device="cuda", generator=gen) + 0.5
    a_, c_ = torch.empty(nb * C, device="cuda"), torch.empty(nb * C, device="cuda")
    _lib.check(lib.gkg_bn_eval_affine(_ptr(gamma), _ptr(beta), _ptr(bias), _ptr(rm), _ptr(rv), _ptr(a_), _ptr(c_), nb * C, eps,
                                      _stream()), "gkg_bn_eval_affine")
    assert float(a_.abs().min()) >= 0.25
    nscale = (R + rps - 1) // rps
    row_scale = (torch.rand(nscale, device="cuda", generator=gen) < 0.7).float() / 0.7 if scaled else None

    def run(form):
        dy = torch.full((nb, R, C), float("nan"), device="cuda")
        outs = [None] * 3 if form == "null" else [torch.full((nb * C,), float("nan"), device="cuda") for _ in range(3)]
        sums = zero_buf = ws = None
        nz = 0
        if form == "atomic":
            sums = torch.zeros(2 * nb * C, dtype=torch.float64, device="cuda")
            zero_buf, nz = torch.ones(50, dtype=torch.float64, device="cuda"), 37
        elif form == "det":
            ws = torch.empty(lib.gkg_bn_workspace_bytes(R, C, nb), dtype=torch.uint8, device="cuda")
        _lib.check(lib.gkg_bn_eval_bwd(_ptr(dout_full), _ptr(Y), _ptr(a_), _ptr(c_), _ptr(dy), R, C, nb, ldg, bstride, act,
                                       _ptr(row_scale), rps if scaled else 0, _ptr(rm), _ptr(rv), _ptr(bias), eps, _ptr(outs[0]),
                                       _ptr(outs[1]), _ptr(outs[2]), _ptr(sums), _ptr(zero_buf), nz, _ptr(ws),
                                       0 if ws is None else ws.numel(), _stream()), "gkg_bn_eval_bwd")
        torch.cuda.synchronize()
        if zero_buf is not None:
            assert float(zero_buf[:nz].abs().max()) == 0.0 and float(zero_buf[nz:].min()) == 1.0      # cleared, and no further
        return dy, outs

    dy, (dgamma, dbeta, dbias) = run("atomic")
    # dY against the fp64 formula
    a64, c64 = a_.double().view(nb, 1, C), c_.double().view(nb, 1, C)
    dout = torch.stack([dout_full[:, q * bstride:q * bstride + C] for q in range(nb)]).double()
    if scaled:
        dout = dout * row_scale.double()[torch.arange(R, device="cuda") // rps].view(1, R, 1)
    z = a64 * Y.double() + c64
    want = a64 * (dout * (_gelu_grad64(z) if act else 1.0))
    err = float((dy.double() - want).abs().max())
    print(f"nb={nb} act={act} scaled={scaled}: dY max |err| {err:.3e}")
    assert torch.allclose(dy.double(), want, atol=2e-4, rtol=1e-3), err

    def check_sums(dgamma, dbeta, dbias, tag):
        dz = dy.double() / a64                                  # the kernel's own dz
        s0, s1 = dz.sum(1).reshape(-1), (dz * Y.double()).sum(1).reshape(-1)
        n0, n1 = dz.abs().sum(1).reshape(-1), (dz * Y.double()).abs().sum(1).reshape(-1)
        sh = bias.double() - rm.double()
        istd = 1.0 / torch.sqrt(rv.double() + float(np.float32(eps)))
        for name, got, exp, bound in (("dbeta", dbeta, s0, 1e-6 * n0),
                                      ("dgamma", dgamma, istd * (s1 + sh * s0), 1e-6 * istd * (n1 + sh.abs() * n0)),
                                      ("dbias", dbias, a_.double() * s0, 1e-6 * a_.double().abs() * n0)):
            ratio = float(((got.double() - exp).abs() / bound).max())
            print(f"  {tag} {name}: max |err| / (1e-6 sum|term|) = {ratio:.3f}")
            assert ratio <= 1.0, (tag, name, ratio)
    check_sums(dgamma, dbeta, dbias, "atomic")
    dy0, _ = run("null")
    assert torch.equal(dy0, dy), "the NULL-sums form must give the same dY bit for bit"
    dy1, det1 = run("det")
    assert torch.equal(dy1, dy)
    check_sums(*det1, "deterministic")
    _, det2 = run("det")
    assert all(torch.equal(p, q) for p, q in zip(det1, det2))


# ------------------------------------------------------------------------------------------------ (5) determinism
def test_deterministic_mode_is_bit_reproducible():
    from gkgnet_amd import fused
    meta, a = load_fixture("f22_frozen_bn")
    old = fused.DETERMINISTIC
    fused.DETERMINISTIC = True
    try:
        runs = []
        for _ in range(2):
            g, gl = _modules(meta, a)
            with _Spy(g) as spy:
                _step(g, gl, a)
            assert spy.calls >= 1 and spy.label_calls >= 1
            _check_param_grads(a, g, gl)
            runs.append([p.grad.clone() for p in list(g.parameters()) + list(gl.parameters()) if p.grad is not None])
    finally:
        fused.DETERMINISTIC = old
    assert len(runs[0]) == len(runs[1]) > 0
    assert all(torch.equal(p, q) for p, q in zip(*runs))


# ------------------------------------------------------------------------------------------------ fused vs composable helper
def _both_paths(meta, a, prepare, seed=None, drop_path=0.0, autocast=False):
    """The same step on the fused and on the composable path (fresh modules each) -> {path: (out, e2, dx, de, grads)}."""
    from gkgnet_amd import fused
    res = {}
    old = fused.ENABLED
    try:
        for name in ("fused", "composable"):
            fused.ENABLED = name == "fused"
            g, gl = _modules(meta, a, drop_path)
            prepare(g, gl)
            if seed is not None:
                torch.manual_seed(seed)
            with _Spy(g) as spy:
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    out, e2, idx, dx, de = _step(g, gl, a)
            assert (spy.calls >= 1 and spy.label_calls >= 1) == (name == "fused")
            grads = {pre + k: p.grad for pre, m in (("g/", g), ("gl/", gl)) for k, p in m.named_parameters() if p.requires_grad}
            res[name] = (out.float(), e2.float(), dx.float(), de.float(), grads)
    finally:
        fused.ENABLED = old
    return res


def _compare_paths(res):
    f, c = res["fused"], res["composable"]
    for name, x, y in zip(("out", "e2", "dx", "de"), f[:4], c[:4]):
        err = float((x - y).abs().max())
        print(f"{name}: fused vs composable max |diff| {err:.3e}")
        assert torch.allclose(x, y, **TOL), (name, err)
    for k, gc in c[4].items():
        gf = f[4][k]
        if gf is None:       # fused path: the bias of a conv feeding TRAIN-mode BN has an identically zero gradient
            assert k.endswith(".0.bias") and (gc is None or float(gc.abs().max()) < 2e-3), k
            continue
        assert torch.allclose(gf, gc, **PTOL), (k, float((gf - gc).abs().max()))


# ------------------------------------------------------------------------------------------------ (6) mixed modes
@pytest.mark.parametrize("train_fc1", [True, False])
def test_mixed_train_and_frozen_layers(train_fc1):
    """fc1's BatchNorm in train mode and every other one frozen, and the reverse: a train-mode producer in front of an
    eval-mode consumer and an eval-mode producer in front of a train-mode consumer, against the composable path."""
    from gkgnet_amd import fused
    meta, a = load_fixture("f22_frozen_bn")

    def prepare(g, gl):
        for mod in (g, gl):
            for m in _bns(mod):
                m.train(m is mod.fc1[1] if train_fc1 else m is not mod.fc1[1])
    old = fused.BN_EPILOGUE_MIN_ROWS
    fused.BN_EPILOGUE_MIN_ROWS = 0           # attach the producer -> consumer BN link at this size too (as the train-mode tests do)
    try:
        res = _both_paths(meta, a, prepare)
    finally:
        fused.BN_EPILOGUE_MIN_ROWS = old
    _compare_paths(res)
    frozen_bias = [k for k in res["fused"][4] if k.endswith(".0.bias") and (k.split("/")[1].startswith("fc1.") != train_fc1)]
    assert frozen_bias and all(res["fused"][4][k] is not None for k in frozen_bias)


# ------------------------------------------------------------------------------------------------ (7) DropPath
def test_frozen_bn_with_active_droppath():
    """drop_path = 0.3 with the same seed on both paths (DropPath.sample_scale consumes the RNG alike): the per-image scale of
    the incoming gradient is applied inside gkg_bn_eval_bwd."""
    meta, a = load_fixture("f22_frozen_bn")
    _compare_paths(_both_paths(meta, a, lambda g, gl: None, seed=7, drop_path=0.3))


# ------------------------------------------------------------------------------------------------ (8) bf16 autocast
def test_frozen_bn_under_bf16_autocast():
    """The frozen step under bf16 autocast (projections on the library GEMM, fp32 Y) does not raise, and the fused and
    composable input gradients lie no further apart than 2 x what the TRAIN-mode BN step shows on the same inputs (the
    project's flip-bound convention, test_hip_modules.py FLIP_BOUND: a bf16 near-tie neighbour flip is discrete).
    Quantity: mean |dx_fused - dx_composable| / mean |dx_fp32| of the same mode.
    Measured on MI355X (EXPERIMENTS.md "Frozen BatchNorm"; both values are printed here): train-mode BN 3.90e-3, frozen BN
    1.31e-3."""
    meta, a = load_fixture("f22_frozen_bn")

    def distance(prepare):
        ref = _both_paths(meta, a, prepare)["fused"][2]
        res = _both_paths(meta, a, prepare, autocast=True)
        assert all(torch.isfinite(t).all() for t in res["fused"][:4])
        return float((res["fused"][2] - res["composable"][2]).abs().mean() / ref.abs().mean())

    def all_train(g, gl):
        for m in _bns(g, gl):
            m.train()
    d_train = distance(all_train)
    d_frozen = distance(lambda g, gl: None)
    print(f"bf16 autocast, mean |dx_fused - dx_composable| / mean |dx_fp32|: train-mode BN {d_train:.4e}, frozen BN {d_frozen:.4e}")
    assert d_frozen <= 2.0 * d_train, (d_frozen, d_train)


# ------------------------------------------------------------------------------------------------ (9) backbone
def _count_eval_bwd(fused):
    """Wraps the eval-mode BN backward (bn_passes._eval_backward, which the fused path's nodes reach through bn_passes.backward)
    with a call counter -> (counter list, restore())."""
    from gkgnet_amd import bn_passes
    real, calls = bn_passes._eval_backward, [0]

    def counted(*args, **kw):
        calls[0] += 1
        return real(*args, **kw)
    bn_passes._eval_backward = counted
    return calls, lambda: setattr(bn_passes, "_eval_backward", real)


@pytest.mark.parametrize("unit", ["stem", "downsample", "ffn"])
def test_backbone_units_with_frozen_bn(unit):
    """The backbone's own units (stem and Downsample: library convolution + BN (+ GELU) on the token-major kernels; FFN: two
    projections) with frozen BatchNorm, fused against composable: output, input gradient and every parameter gradient."""
    from gkgnet_amd import fused
    from gkgnet_amd.backbone import FFN, Downsample, Stem
    make, shape = {"stem": (lambda: Stem(out_dim=48, act="gelu"), (2, 3, 64, 64)),
                   "downsample": (lambda: Downsample(48, 96), (2, 48, 16, 16)),
                   "ffn": (lambda: FFN(48, 192, act="gelu"), (2, 48, 16, 16))}[unit]
    torch.manual_seed(3)
    proto = make()
    with torch.no_grad():
        for m in _bns(proto):
            m.weight.uniform_(0.5, 1.5)
            m.bias.normal_(0.0, 0.1)
            m.running_mean.normal_(0.0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
        for m in proto.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.bias.normal_(0.0, 0.1)
    sd = proto.state_dict()
    x0, res = torch.randn(shape, device="cuda"), {}
    old = fused.ENABLED
    try:
        for name in ("fused", "composable"):
            fused.ENABLED = name == "fused"
            mod = make()
            mod.load_state_dict(sd)
            mod.cuda().train()
            for m in _bns(mod):
                m.eval()
            before = _buffers(mod)
            x = x0.clone().requires_grad_(True)
            if unit != "stem":
                x = x0.clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
            calls, restore = _count_eval_bwd(fused)
            try:
                out = mod(x)
                if "cot" not in res:
                    res["cot"] = torch.randn(out.shape, device="cuda")
                (out * res["cot"]).sum().backward()
            finally:
                restore()
            assert (calls[0] > 0) == (name == "fused"), (name, calls[0])
            assert all(torch.equal(p, q) for p, q in zip(before, _buffers(mod)))
            res[name] = (out.detach(), x.grad, {k: p.grad for k, p in mod.named_parameters()})
    finally:
        fused.ENABLED = old
    f, c = res["fused"], res["composable"]
    for name, p, q in (("out", f[0], c[0]), ("dx", f[1], c[1])):
        err = float((p - q).abs().max())
        print(f"{unit} {name}: fused vs composable max |diff| {err:.3e}")
        assert torch.allclose(p, q, **TOL), (name, err)
    for k, gc in c[2].items():
        assert f[2][k] is not None, k
        assert torch.allclose(f[2][k], gc, **PTOL), (k, float((f[2][k] - gc).abs().max()))


def test_tiny_backbone_norm_eval_two_sgd_steps():
    """GKGNet(norm_eval=True) at the F10 size: two plain-SGD steps (lr 1e-3) on the fused path run, leave every BN buffer
    untouched, and end at the composable path's loss to 1e-3 relative.  Loss: fixed random cotangents on the backbone's two
    floating-point outputs (label tokens, pooled feature).

    Weights: what a fine-tuning run starts from — a network whose running statistics describe its own activations.  The
    backbone's default initialisation, then 40 train-mode forward passes (no gradients) so that every BatchNorm's running
    mean / variance have converged to the statistics of the input batch (momentum 0.1: 0.9^40 = 1.5 %), and only then the
    freeze.  F10's keyed_fill_ weights do not serve: with them the activations reach ~200 (test_backbone.py) and, BN no longer
    renormalising, one lr = 1e-3 SGD step sends BOTH paths to NaN (measured on MI355X: -6129.7 / -5795.5 at step 0, then NaN).
    Cotangents: N(0, 1) / numel of their output, i.e. a loss of mean-reduced size (gradient norm ~20, so a step moves the
    weights by ~2e-2); with unit cotangents the gradient norm is ~2e4 and one step overwrites the weights on both paths.
    Seed: the case must be free of fp32 near-tie neighbour flips BETWEEN the two paths in all three forward passes, like every
    fixture (tests/util.py NEAR_TIE): the two paths round fc1 differently in the last bit, one flipped neighbour out of 23 808
    slots re-routes gradients (1e-2 relative on that block's fc1 weight) and the 14 graph layers behind it amplify that.
    Measured on MI355X over seeds 6..59 at B = 1: 21 seeds are flip-free and ALL of them end within 5e-5 relative (seed 26:
    1.7e-6); the 33 with a flip end 5e-2 .. 6 apart — with identical graphs every parameter gradient of the backbone agrees
    between the paths to 2.5e-5 of its maximum.  Seed 26 is one of the flip-free ones."""
    from gkgnet_amd import fused
    from gkgnet_amd.backbone import GKGNet
    meta, _ = load_fixture("f10_backbone_tiny")
    seed = 26
    gen = torch.Generator(device="cuda").manual_seed(seed)
    img = torch.randn(1, 3, meta["ctor"]["size"], meta["ctor"]["size"], device="cuda", generator=gen)
    torch.manual_seed(seed)
    proto = GKGNet(**meta["ctor"]).cuda().train()
    with torch.no_grad():
        for _ in range(40):
            proto(img)
    sd = {k: v.detach().clone() for k, v in proto.state_dict().items()}
    cots = None
    losses = {}
    old = fused.ENABLED
    try:
        for name in ("fused", "composable"):
            fused.ENABLED = name == "fused"
            net = GKGNet(**meta["ctor"], norm_eval=True)
            net.load_state_dict(sd)
            net.cuda().train()
            assert all(not m.training for m in _bns(net))
            before = _buffers(net)
            opt = torch.optim.SGD(net.parameters(), lr=1e-3)
            graphers, real = [0], fused.grapher_forward

            def spy(*args, **kw):
                graphers[0] += 1
                return real(*args, **kw)
            fused.grapher_forward = spy
            calls, restore = _count_eval_bwd(fused)
            try:
                losses[name] = []
                for it in range(3):                      # two updates, then the loss they lead to
                    labels, gap, _ = net(img)
                    if cots is None:
                        cots = (torch.randn(labels.shape, device="cuda", generator=gen) / labels.numel(),
                                torch.randn(gap.shape, device="cuda", generator=gen) / gap.numel())
                    loss = (labels * cots[0]).sum() + (gap * cots[1]).sum()
                    if it < 2:
                        opt.zero_grad(set_to_none=True)
                        loss.backward()
                        opt.step()
                    losses[name].append(float(loss.detach()))
            finally:
                fused.grapher_forward = real
                restore()
            assert (graphers[0] > 0) == (name == "fused") and (calls[0] > 0) == (name == "fused")
            assert all(torch.equal(x, y) for x, y in zip(before, _buffers(net))), "a frozen BN buffer changed"
    finally:
        fused.ENABLED = old
    print("losses (step 0, step 1, after step 2):", losses)
    lf, lc = losses["fused"][2], losses["composable"][2]
    assert all(math.isfinite(v) for v in losses["fused"] + losses["composable"])
    assert abs(lf - lc) <= 1e-3 * abs(lc), (lf, lc)


# ------------------------------------------------------------------------------------------------ (10) hipGraph capture
def test_frozen_bn_step_captures_into_a_graph():
    """No host synchronisation in the frozen-BN backward: a Grapher -> GrapherLabel SGD step with frozen BatchNorm (gradient
    bucket, in-graph optimiser step; gamma / beta still trained) captures into GraphedStep and its replays follow the eager
    steps batch after batch, at the tolerances test_hip_graphed_step.py applies to the train-mode step."""
    from gkgnet_amd import parallel
    from gkgnet_amd.graphed import GraphedStep
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    from gkgnet_amd.layers import freeze_batchnorm
    C, H, L, B = 64, 12, 20, 4

    def build():
        torch.manual_seed(3)
        g = Grapher(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=True, use_multi_group=True,
                    num_group=2).cuda()
        gl = GrapherLabel(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=False, num_nodes=L,
                          use_multi_group=True, num_group=2).cuda()
        with torch.no_grad():
            for m in _bns(g, gl):
                m.running_mean.normal_(0.0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
        freeze_batchnorm(g, affine=True).train()
        freeze_batchnorm(gl, affine=True).train()
        assert all(not m.training for m in _bns(g, gl))
        params = [p for p in list(g.parameters()) + list(gl.parameters()) if p.requires_grad]
        bucket = parallel.GradBucket(params)
        opt = torch.optim.SGD(params, lr=0.01)
        x, e = torch.zeros(B, C, H, H, device="cuda"), torch.zeros(B, L, C, device="cuda")
        loss = torch.zeros((), device="cuda")

        def step():
            bucket.release(prezero=True)
            out = g(x)
            e2, _ = gl(e, out)
            val = (out.float() ** 2).mean() + (e2.float() ** 2).mean()
            val.backward()
            bucket.pack()
            opt.step()
            loss.copy_(val.detach())
        return g, gl, params, x, e, loss, step
    gen = torch.Generator(device="cuda").manual_seed(11)
    data = [(torch.randn(B, C, H, H, device="cuda", generator=gen), torch.randn(B, L, C, device="cuda", generator=gen))
            for _ in range(5)]
    g, gl, params, x, e, loss, step = build()
    before = _buffers(g, gl)
    x.copy_(data[0][0]); e.copy_(data[0][1])
    for _ in range(3):
        step()
    ref = []
    for bx, be in data[1:]:
        x.copy_(bx); e.copy_(be)
        step()
        ref.append(float(loss))
    ref_w = [p.detach().clone() for p in params]
    assert all(torch.equal(p, q) for p, q in zip(before, _buffers(g, gl)))
    g2, gl2, params2, x2, e2, loss2, step2 = build()
    x2.copy_(data[0][0]); e2.copy_(data[0][1])
    gs = GraphedStep(step2, warmup=3)
    assert gs.captured, "the frozen-BN step must capture"
    got = []
    for bx, be in data[1:]:
        x2.copy_(bx); e2.copy_(be)
        gs.replay()
        got.append(float(loss2))
    print("eager", ref, "replayed", got)
    for a_, b_ in zip(got, ref):
        assert abs(a_ - b_) <= 2e-3 * abs(b_) + 1e-6, (got, ref)
    for p, q in zip(params2, ref_w):
        assert float((p.detach() - q).abs().max()) <= 2e-3 * float(q.abs().max()) + 1e-5
    assert all(torch.equal(p, q) for p, q in zip(before, _buffers(g2, gl2)))
