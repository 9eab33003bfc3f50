"""GKG_ENABLE=train_bf16 at module level: one Grapher + FFN pair in train mode under bf16 autocast with gradients (reference
torch_vertex.py:290-333, gkgnet.py:46-72) — which launches the four dense layers make with the switch on and off, what stays
bit-identical, how close the gradients stay to the fp32 step next to torch's own mixed precision, and that parameter updates reach
the kernels' weight fragments.

Sizes: C = 48 (a partial 32-column block in every layer: 48, 96, 192 columns), G = 2, 9 x 9 tokens, B = 2 -> R = 162 rows (one
full 128-row tile and a partial one), k = 4."""
import pytest
import torch

from tests.test_hip_linear_bf16 import _definition, _TorchProxy
from tests.util import keyed_fill_

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
C, G, H, K, B = 48, 2, 9, 4, 2
DENSE = ("g.fc1.0.weight", "g.fc2.0.weight", "ffn.fc1.0.weight", "ffn.fc2.0.weight")


def _pair():
    """Fresh modules with the same keyed parameters every time (nothing cached on them from another run)."""
    from gkgnet_amd import layers
    from gkgnet_amd.backbone import FFN
    from gkgnet_amd.grapher import Grapher
    layers.norm_cfg["type"] = "BN"
    g = Grapher(C, K, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, drop_path=0.0, relative_pos=True,
                use_multi_group=True, num_group=G)
    ffn = FFN(C, 4 * C, act="gelu")
    for i, m in enumerate((g, ffn)):
        sd = m.state_dict()
        keyed_fill_(sd, seed=40 + i)
        m.load_state_dict(sd)
        m.cuda().train()
    return g, ffn


def _inputs():
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, H, H, generator=gen).cuda().to(memory_format=torch.channels_last)
    cot = torch.randn(B, C, H, H, generator=gen).cuda()
    return x, cot


def _step(g, ffn, x, cot, amp=BF16):
    """Forward + backward of the pair -> (out, dx, {name: grad})."""
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    for m in (g, ffn):
        m.zero_grad(set_to_none=True)
    if amp is None:
        out = ffn(g(x))
    else:
        with torch.autocast("cuda", dtype=amp):
            out = ffn(g(x))
    (out.float() * cot).sum().backward()
    grads = {f"{n}.{k}": p.grad.detach().clone() for n, m in (("g", g), ("ffn", ffn)) for k, p in m.named_parameters()
             if p.grad is not None}
    return out.detach().float(), x.grad.detach().clone(), grads


def _same_bits(a, b):
    (oa, da, ga), (ob, db, gb) = a, b
    assert torch.equal(oa, ob) and torch.equal(da, db)
    assert ga.keys() == gb.keys()
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def _instrument(monkeypatch):
    """Counting wrappers around the three own callers of ``fused`` (recording operands and results of the bf16 kind, without the kind
    argument), the library GEMMs of ``fused`` and gkg_linear_wgrad_x6 (recording nb)."""
    from gkgnet_amd import _lib, fused
    rec, counts, x6 = {"fwd": [], "dgrad": [], "wgrad": []}, {}, []
    for key, name in (("fwd", "train16_fwd"), ("dgrad", "train16_dgrad"), ("wgrad", "linear_bf16_wgrad")):
        def recording(*a, _real=getattr(fused, name), _key=key, **k):
            out = _real(*a, **k)
            if _key == "wgrad":
                rec[_key].append((a, k, out))
            elif a[0].name == "bf16":
                rec[_key].append((a[1:], k, out))
            return out
        monkeypatch.setattr(fused, name, recording)
    lib = _lib.load()
    real_x6 = lib.gkg_linear_wgrad_x6

    def counted(*a):
        x6.append(a[10])                                                         # nb
        return real_x6(*a)
    monkeypatch.setattr(lib, "gkg_linear_wgrad_x6", counted)
    monkeypatch.setattr(fused, "torch", _TorchProxy(counts))
    return rec, counts, x6


def test_dispatch_with_the_switch_on_and_off(monkeypatch):
    from gkgnet_amd import fused
    assert hasattr(fused, "TRAIN_BF16")
    x, cot = _inputs()
    rec, counts, x6 = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "TRAIN_BF16", False)
    off1 = _step(*_pair(), x, cot)
    assert not any(rec.values())
    gemm_off = counts.get("mm", 0) + counts.get("addmm", 0)
    x6_off = list(x6)
    counts.clear()
    x6.clear()
    monkeypatch.setattr(fused, "TRAIN_BF16", True)
    on = _step(*_pair(), x, cot)
    gemm_on = counts.get("mm", 0) + counts.get("addmm", 0)
    print(f"own launches: {[len(v) for v in rec.values()]}; library GEMMs of fused off {gemm_off} on {gemm_on}; "
          f"x6 weight gradients (nb) off {x6_off} on {x6}")
    assert [len(rec[k]) for k in ("fwd", "dgrad", "wgrad")] == [4, 4, 4]
    assert gemm_off - gemm_on == 8 and gemm_on == 0          # 4 forward mm + 4 input-gradient mm / addmm, none left
    assert sorted(x6_off) == [1, 1, 1, 1, 4] and x6 == [4]   # only the grouped projection's weight gradient stays on x6
    for t in (on[0], on[1], *on[2].values()):
        assert bool(torch.isfinite(t).all())
    for k in rec:
        rec[k].clear()
    monkeypatch.setattr(fused, "TRAIN_BF16", False)
    off2 = _step(*_pair(), x, cot)
    assert not any(rec.values())
    _same_bits(off1, off2)


@pytest.mark.parametrize("case", ["fp16", "deterministic", "fp32"])
def test_out_of_scope_steps_keep_their_bits(case, monkeypatch):
    from gkgnet_amd import fused
    x, cot = _inputs()
    rec, _, _ = _instrument(monkeypatch)
    if case == "deterministic":
        monkeypatch.setattr(fused, "DETERMINISTIC", True)
    amp = {"fp16": torch.float16, "deterministic": BF16, "fp32": None}[case]
    got = {}
    for on in (False, True):
        monkeypatch.setattr(fused, "TRAIN_BF16", on)
        got[on] = _step(*_pair(), x, cot, amp=amp)
        assert not any(rec.values()), case
    _same_bits(got[False], got[True])


def _label():
    from gkgnet_amd import layers
    from gkgnet_amd.grapher import GrapherLabel
    layers.norm_cfg["type"] = "BN"
    gl = GrapherLabel(C, K, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, drop_path=0.0, relative_pos=False,
                      num_nodes=20, use_multi_group=True, num_group=G)
    sd = gl.state_dict()
    keyed_fill_(sd, seed=42)
    gl.load_state_dict(sd)
    return gl.cuda().train()


def test_label_block_route_keeps_the_grouped_layer_on_its_path(monkeypatch):
    """A whole GrapherLabel forward + backward under bf16 autocast, through ``_lin`` and the predicate: with the switch on its four
    DENSE layers (fc1, fc2, ffn.fc1, ffn.fc2 — the alias forms, whose skip gradient rides in the input gradient's epilogue) take
    the own kernels, every own launch belongs to a groups = 1 layer, and the grouped projection keeps gkg_linear_wgrad_x6 (nb = 4)
    and makes no own launch."""
    from gkgnet_amd import fused
    rec, counts, x6 = _instrument(monkeypatch)
    gen = torch.Generator().manual_seed(9)
    e0 = torch.randn(B, 20, C, generator=gen).cuda()
    feats = torch.randn(B, C, H, H, generator=gen).cuda().to(memory_format=torch.channels_last)
    cot = torch.randn(B, 20, C, generator=gen).cuda()
    got = {}
    for on in (False, True):
        monkeypatch.setattr(fused, "TRAIN_BF16", on)
        x6.clear()
        gl = _label()
        e = e0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF16):
            out, _ = gl(e, feats)
        (out.float() * cot).sum().backward()
        got[on] = (out.detach().float(), e.grad.clone(), list(x6), gl)
        if not on:
            assert not any(rec.values())
    out_on, de_on, x6_on, gl = got[True]
    print(f"label block: own launches {[len(v) for v in rec.values()]}, x6 weight gradients (nb) off {got[False][2]} on {x6_on}")
    assert [len(rec[k]) for k in ("fwd", "dgrad", "wgrad")] == [4, 4, 4]
    dense = {id(m[0]) for m in (gl.fc1, gl.fc2, gl.ffn.fc1, gl.ffn.fc2)}
    assert {id(a[1]) for a, _, _ in rec["fwd"]} == dense and all(a[1].groups == 1 for a, _, _ in rec["fwd"])
    assert {id(a[1]) for a, _, _ in rec["dgrad"]} == dense
    assert sum(1 for _, k, _ in rec["dgrad"] if k.get("residual") is not None) >= 2      # fc1's and ffn.fc1's alias gradients
    assert x6_on == [4] and sorted(got[False][2]) == [1, 1, 1, 1, 4]
    for t_on, t_off, what in ((out_on, got[False][0], "output"), (de_on, got[False][1], "input gradient")):
        assert bool(torch.isfinite(t_on).all())
        print(f"  {what}: mean relative difference to the switch-off run "
              f"{((t_on - t_off).abs().mean() / t_off.abs().mean()).item():.3e}")
    # (printed, not bounded: switched off, the autocast GEMM rounds Y itself to bf16 and the label graph is free to flip
    # neighbours on that, so the two runs are not one computation in two summation orders; how close the switch-on gradients
    # stay to fp32 is the yardstick test's, on forced graphs.)


def test_grouped_projection_keeps_its_bits(monkeypatch):
    """A GrapherLabel's grouped layer (Conv2d 1x1 groups = 4 + BN + GELU on the [x | m] operand buffer) under bf16 autocast, called
    as the Function itself on a fixed operand buffer — inside a block its input comes from fc1, whose rounding the switch changes,
    so only the isolated call can be compared bit for bit.  What this pins is narrow: ``_GroupedLinearBNAct`` reads nothing of
    the switch (flipping the module constant changes no bit and adds no launch); that the grouped layer is never ROUTED to the own
    kernels is test_label_block_route_keeps_the_grouped_layer_on_its_path's and the dispatch test's ``x6 == [4]``."""
    from gkgnet_amd import fused, layers
    from gkgnet_amd.grapher import GrapherLabel
    layers.norm_cfg["type"] = "BN"
    rec, _, _ = _instrument(monkeypatch)
    gen = torch.Generator().manual_seed(3)
    XM0 = torch.randn(B * 20, 2 * C, generator=gen).cuda()
    cot = torch.randn(B * 20, 2 * C, generator=gen).cuda()
    got = {}
    for on in (False, True):
        monkeypatch.setattr(fused, "TRAIN_BF16", on)
        gl = GrapherLabel(C, K, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, drop_path=0.0, relative_pos=False,
                          num_nodes=20, use_multi_group=True, num_group=G)
        sd = gl.state_dict()
        keyed_fill_(sd, seed=42)
        gl.load_state_dict(sd)
        gl.cuda().train()
        conv, bn = gl.graph_conv.gconv.nn[0], gl.graph_conv.gconv.nn[1]
        assert conv.groups == 4
        XM = XM0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF16):
            out = fused._GroupedLinearBNAct.apply(XM, conv.weight, conv.bias, bn.weight, bn.bias, bn, 1, False, None)
        (out.float() * cot).sum().backward()
        got[on] = (out.detach(), XM.grad.clone(), conv.weight.grad.clone(), bn.weight.grad.clone())
        assert not any(rec.values())
    for a, b in zip(got[False], got[True]):
        assert torch.equal(a, b)


def test_gradients_stay_as_close_to_fp32_as_torch_autocast_does(monkeypatch):
    """Yardstick: torch's own mixed precision — the same modules on the composable path (fused.ENABLED = False), whose 1x1
    convolutions torch runs in bf16 forward and backward under autocast.  The fp32 run's neighbour graph is forced into both
    autocast runs, so no near-tie flip enters.  For dx and the four dense weights' gradients, e = mean|g - g_fp32| / mean|g_fp32|:
    required e_on <= 1.5 e_composable (the factor of test_hip_linear_bf16.py and F14)."""
    from gkgnet_amd import fused, ops
    x, cot = _inputs()
    edges = []
    real_tm, real_ops = fused.knn_graph_tm, ops.knn_graph

    def recording(*a, **k):
        e = real_tm(*a, **k)
        edges.append(e)
        return e
    monkeypatch.setattr(fused, "TRAIN_BF16", False)
    monkeypatch.setattr(fused, "knn_graph_tm", recording)
    ref = _step(*_pair(), x, cot, amp=None)
    assert len(edges) == 1
    edge = edges[0]

    def forced_tm(*a, **k):
        return edge

    def forced_ops(*a, **k):
        own = real_ops(*a, **k)
        assert own.shape == edge.shape and own.dtype == edge.dtype
        return edge
    monkeypatch.setattr(fused, "knn_graph_tm", forced_tm)
    monkeypatch.setattr(ops, "knn_graph", forced_ops)
    monkeypatch.setattr(fused, "ENABLED", False)
    comp = _step(*_pair(), x, cot)
    monkeypatch.setattr(fused, "ENABLED", True)
    rec, _, _ = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "TRAIN_BF16", True)
    on = _step(*_pair(), x, cot)
    assert len(rec["fwd"]) == 4

    def e(run, name):
        g, r = (run[1], ref[1]) if name == "dx" else (run[2][name], ref[2][name])
        return ((g.double() - r.double()).abs().mean() / r.double().abs().mean()).item()
    for name in ("dx",) + DENSE:
        e_on, e_comp = e(on, name), e(comp, name)
        print(f"{name}: mean|g - g_fp32| / mean|g_fp32|  train_bf16 {e_on:.4e}  composable autocast {e_comp:.4e}")
    for name in ("dx",) + DENSE:
        assert e(on, name) <= 1.5 * e(comp, name), (name, e(on, name), e(comp, name))


def test_two_sgd_steps_rebuild_the_fragments(monkeypatch):
    from gkgnet_amd import derived, fused
    x, cot = _inputs()
    rec, _, _ = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "TRAIN_BF16", True)
    g, ffn = _pair()
    params = [p for m in (g, ffn) for p in m.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=0.05)
    conv = ffn.fc1[0]
    planes, w_at = [], []
    for _ in range(2):
        for k in rec:
            rec[k].clear()
        w_at.append(conv.weight.detach().clone())
        out, dx, grads = _step(g, ffn, x, cot)
        planes.append((derived.peek(conv, "lin_planes"), derived.peek(conv, "lin_planes_t")))
        for t in (out, dx, *grads.values()):
            assert bool(torch.isfinite(t).all())
        opt.step()
    assert not torch.equal(w_at[0], w_at[1])
    assert planes[0][0] is not planes[1][0] and planes[0][1] is not planes[1][1]
    assert not torch.equal(planes[0][0], planes[1][0]) and not torch.equal(planes[0][1], planes[1][1])
    # the second step's forward launch of FFN.fc1 read the weights the first step left: its Y holds the fp64 definition's bound
    # with those weights, and not with the initial ones
    (a, k, Y), = [r for r in rec["fwd"] if r[0][1] is conv]
    xd = a[0].detach().to(BF16).double().cpu()
    holds = {}
    for tag, w in (("second step's weights", w_at[1]), ("initial weights", w_at[0])):
        wd = w.reshape(w.shape[0], -1).to(BF16).double().cpu()
        want, bound = _definition(xd @ wd.t(), xd.abs() @ wd.abs().t(), xd.shape[1], None, torch.zeros(wd.shape[0]), None, 0)
        err = (Y.double().cpu() - want).abs()
        holds[tag] = bool((err <= bound).all())
        print(f"FFN.fc1 second step against the {tag}: max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert holds["second step's weights"] and not holds["initial weights"]
