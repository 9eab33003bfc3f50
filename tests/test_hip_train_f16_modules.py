"""GKG_ENABLE=train_f16 at module level: one Grapher + FFN pair in train mode under fp16 autocast with gradients (reference
torch_vertex.py:290-333, gkgnet.py:46-72; the recipe configs/gkgnet/gkgnet_coco_576.py:146 fp16 = dict(loss_scale='dynamic')) — which
launches the four dense layers make with the switch on and off, what stays bit-identical, that GKG_DETERMINISTIC keeps the switch
and gives run-independent bits, how close the gradients stay to the fp32 step next to torch's own fp16 mixed precision and next to
train_bf16, that parameter updates reach the kernels' weight fragments, and the F17 fixture's train step and overflow behaviour
with the switch on.

Sizes and helpers: tests/test_hip_train_bf16_modules.py (C 48, G 2, 9 x 9 tokens, B 2 -> 162 rows, k 4)."""
import numpy as np
import pytest
import torch

from tests.test_hip_linear_bf16 import _definition, _TorchProxy
from tests.test_hip_train_bf16_modules import DENSE, _inputs, _pair, _same_bits, _step

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
OWN = (("fwd", "train16_fwd"), ("dgrad", "train16_dgrad"), ("wgrad", "linear_bf16_wgrad"))
KEYS = ("f16_fwd", "f16_dgrad", "bf16_fwd", "bf16_dgrad", "bf16_wgrad")


def _instrument(monkeypatch):
    """Recording wrappers around the own callers of ``fused``, sorted by their kind argument (both kinds; recorded without it), the
    library GEMMs of ``fused`` counted, and gkg_linear_wgrad_x6's nb recorded."""
    from gkgnet_amd import _lib, fused
    rec, counts, x6 = {key: [] for key in KEYS}, {}, []
    for what, name in OWN:
        def recording(*a, _real=getattr(fused, name), _what=what, **k):
            out = _real(*a, **k)
            if _what == "wgrad":
                rec["bf16_wgrad"].append((a, k, out))
            else:
                rec[f"{a[0].name}_{_what}"].append((a[1:], k, out))
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


def _lens(rec):
    return {k: len(v) for k, v in rec.items() if v}


def _clear(rec):
    for v in rec.values():
        v.clear()


def test_dispatch_with_the_switch_on_and_off(monkeypatch):
    from gkgnet_amd import fused
    assert hasattr(fused, "TRAIN_F16")
    x, cot = _inputs()
    rec, counts, x6 = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "TRAIN_BF16", False)
    monkeypatch.setattr(fused, "TRAIN_F16", False)
    off1 = _step(*_pair(), x, cot, amp=F16)
    assert not _lens(rec)
    gemm_off = counts.get("mm", 0) + counts.get("addmm", 0)
    x6_off = list(x6)
    counts.clear()
    x6.clear()
    monkeypatch.setattr(fused, "TRAIN_F16", True)
    on = _step(*_pair(), x, cot, amp=F16)
    gemm_on = counts.get("mm", 0) + counts.get("addmm", 0)
    print(f"own launches: {_lens(rec)}; library GEMMs of fused off {gemm_off} on {gemm_on}; x6 weight gradients (nb) off {x6_off} on {x6}")
    assert _lens(rec) == {"f16_fwd": 4, "f16_dgrad": 4}
    assert gemm_off - gemm_on == 8 and gemm_on == 0          # 4 forward mm + 4 input-gradient mm / addmm, none left
    assert sorted(x6_off) == [1, 1, 1, 1, 4] and sorted(x6) == sorted(x6_off)      # the weight gradients stay where they were
    for t in (on[0], on[1], *on[2].values()):
        assert bool(torch.isfinite(t).all())
    _clear(rec)
    monkeypatch.setattr(fused, "TRAIN_F16", False)
    off2 = _step(*_pair(), x, cot, amp=F16)
    assert not _lens(rec)
    _same_bits(off1, off2)


@pytest.mark.parametrize("case", ["bf16", "fp32"])
def test_out_of_scope_steps_keep_their_bits(case, monkeypatch):
    from gkgnet_amd import fused
    x, cot = _inputs()
    rec, _, _ = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "TRAIN_BF16", False)
    amp = {"bf16": BF16, "fp32": None}[case]
    got = {}
    for on in (False, True):
        monkeypatch.setattr(fused, "TRAIN_F16", on)
        got[on] = _step(*_pair(), x, cot, amp=amp)
        assert not _lens(rec), case
    _same_bits(got[False], got[True])


def test_both_switches_on_each_acts_under_its_own_dtype(monkeypatch):
    from gkgnet_amd import fused
    x, cot = _inputs()
    rec, _, _ = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "TRAIN_BF16", True)
    monkeypatch.setattr(fused, "TRAIN_F16", True)
    _step(*_pair(), x, cot, amp=F16)
    assert _lens(rec) == {"f16_fwd": 4, "f16_dgrad": 4}
    _clear(rec)
    _step(*_pair(), x, cot, amp=BF16)
    assert _lens(rec) == {"bf16_fwd": 4, "bf16_dgrad": 4, "bf16_wgrad": 4}
    _clear(rec)
    _step(*_pair(), x, cot, amp=None)
    assert not _lens(rec)


def test_deterministic_keeps_the_switch_and_repeats_its_bits(monkeypatch):
    from gkgnet_amd import fused
    x, cot = _inputs()
    rec, _, _ = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "DETERMINISTIC", True)
    monkeypatch.setattr(fused, "TRAIN_F16", True)
    runs = []
    for _ in range(2):
        _clear(rec)
        runs.append(_step(*_pair(), x, cot, amp=F16))
        assert _lens(rec) == {"f16_fwd": 4, "f16_dgrad": 4}
    (o1, d1, g1), (o2, d2, g2) = runs
    assert torch.equal(o1, o2) and torch.equal(d1, d2)
    for name in DENSE:
        assert torch.equal(g1[name], g2[name]), name
    for t in (o1, d1, *g1.values()):
        assert bool(torch.isfinite(t).all())


def test_gradients_stay_as_close_to_fp32_as_torch_autocast_does(monkeypatch):
    """Yardstick: torch's own fp16 mixed precision — the same modules on the composable path (fused.ENABLED = False), whose 1x1
    convolutions torch runs in fp16 forward and backward under autocast.  The fp32 run's neighbour graph is forced into every
    autocast run, so no near-tie flip enters.  For dx and the four dense weights' gradients, e = mean|g - g_fp32| / mean|g_fp32|:
    required e_f16 <= 1.5 e_composable (the project's factor: test_hip_train_bf16_modules.py, F14) AND e_f16 <= e_bf16, the
    train_bf16 figure of the same quantity measured here (operand rounding unit 2^-11 against 2^-8, same kernel otherwise)."""
    from gkgnet_amd import fused, ops
    x, cot = _inputs()
    edges = []
    real_tm, real_ops = fused.knn_graph_tm, ops.knn_graph

    def recording(*a, **k):
        e = real_tm(*a, **k)
        edges.append(e)
        return e
    monkeypatch.setattr(fused, "TRAIN_BF16", False)
    monkeypatch.setattr(fused, "TRAIN_F16", False)
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
    comp = _step(*_pair(), x, cot, amp=F16)
    monkeypatch.setattr(fused, "ENABLED", True)
    rec, _, _ = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "TRAIN_F16", True)
    on = _step(*_pair(), x, cot, amp=F16)
    assert _lens(rec) == {"f16_fwd": 4, "f16_dgrad": 4}
    monkeypatch.setattr(fused, "TRAIN_F16", False)
    off = _step(*_pair(), x, cot, amp=F16)
    monkeypatch.setattr(fused, "TRAIN_BF16", True)
    _clear(rec)
    b16 = _step(*_pair(), x, cot, amp=BF16)
    assert len(rec["bf16_fwd"]) == 4

    def e(run, name):
        g, r = (run[1], ref[1]) if name == "dx" else (run[2][name], ref[2][name])
        return ((g.double() - r.double()).abs().mean() / r.double().abs().mean()).item()
    for name in ("dx",) + DENSE:
        print(f"{name}: mean|g - g_fp32| / mean|g_fp32|  train_f16 {e(on, name):.4e}  switch off {e(off, name):.4e}  "
              f"composable fp16 autocast {e(comp, name):.4e} (ratio {e(on, name) / e(comp, name):.3f})  train_bf16 {e(b16, name):.4e} "
              f"(ratio {e(on, name) / e(b16, name):.3f})")
    for name in ("dx",) + DENSE:
        assert e(on, name) <= 1.5 * e(comp, name), (name, e(on, name), e(comp, name))
        assert e(on, name) <= e(b16, name), (name, e(on, name), e(b16, name))


def test_parameter_updates_rebuild_the_fragments(monkeypatch):
    """Step, optimizer step + mark_parameters_updated, step, optimizer step WITHOUT the mark (the version counters see the in-place
    update), step: each forward streams the fragments of the weights it was called with."""
    from gkgnet_amd import derived, fused
    x, cot = _inputs()
    rec, _, _ = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "TRAIN_F16", True)
    g, ffn = _pair()
    params = [p for m in (g, ffn) for p in m.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=0.05)
    conv = ffn.fc1[0]
    planes, w_at, ys = [], [], []
    for i in range(3):
        _clear(rec)
        w_at.append(conv.weight.detach().clone())
        out, dx, grads = _step(g, ffn, x, cot, amp=F16)
        planes.append((derived.peek(conv, "lin_planes_f16"), derived.peek(conv, "lin_planes_t_f16")))
        ys.append([r for r in rec["f16_fwd"] if r[0][1] is conv])
        for t in (out, dx, *grads.values()):
            assert bool(torch.isfinite(t).all())
        opt.step()
        if i == 0:
            fused.mark_parameters_updated()
    for i in (1, 2):
        assert not torch.equal(w_at[i - 1], w_at[i])
        assert planes[i][0] is not planes[i - 1][0] and planes[i][1] is not planes[i - 1][1]
        assert not torch.equal(planes[i][0], planes[i - 1][0]) and not torch.equal(planes[i][1], planes[i - 1][1])
        # this step's forward launch of FFN.fc1 read the weights the step before left: its Y holds the fp64 definition's bound with
        # those weights, and not with the previous ones
        (a, k, Y), = ys[i]
        xd = a[0].detach().to(F16).double().cpu()
        holds = {}
        for tag, w in (("current", w_at[i]), ("previous", w_at[i - 1])):
            wd = w.reshape(w.shape[0], -1).to(F16).double().cpu()
            want, bound = _definition(xd @ wd.t(), xd.abs() @ wd.abs().t(), xd.shape[1], None, torch.zeros(wd.shape[0]), None, 0)
            err = (Y.double().cpu() - want).abs()
            holds[tag] = bool((err <= bound).all())
            print(f"FFN.fc1 step {i} against the {tag} weights: max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert holds["current"] and not holds["previous"]


# ------------------------------------------------------------------------------------------------ F17 with the switch on
def _f17():
    from tests.test_hip_autocast_trainstep import _amp_modules, _set_agreement, _t
    from tests.util import load_fixture
    meta, a = load_fixture("f17_amp_fp16")
    return meta, a, _amp_modules, _set_agreement, _t


def test_f17_train_step_meets_its_bar_with_the_switch_on(monkeypatch):
    """tests/test_hip_autocast_trainstep.py::test_amp_fp16_train_step_against_reference_fp16_fixture's step and bar — every output
    and gradient at least as close to the reference's fp32 result as the reference's own fp16-autocast run (+ 1e-6), label
    neighbour sets agreeing with the fp32 reference at least as well as the reference's fp16 run — with GKG_ENABLE=train_f16."""
    from gkgnet_amd import fused
    meta, a, _amp_modules, _set_agreement, _t = _f17()
    assert meta["finite"]
    rec, counts, _ = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "TRAIN_F16", True)
    g, gl = _amp_modules(meta, a)
    S = meta["loss_scale"]
    x = _t(a["x"]).requires_grad_(True)
    e = _t(a["e"]).requires_grad_(True)
    with torch.autocast("cuda", dtype=F16):
        out = g(x)
        e2, idx = gl(e, out)
    loss = ((out.float() * _t(a["cot_x"])).sum() + (e2.float() * _t(a["cot_e"])).sum()) * S
    loss.backward()
    print(f"F17 own launches: {_lens(rec)}, library GEMMs of fused: {dict(counts)}")
    assert len(rec["f16_fwd"]) >= 4 and len(rec["f16_dgrad"]) >= 4 and not rec["bf16_fwd"]
    got = dict(out=out.detach().float(), labels=e2.detach().float(), dx=x.grad / S, de=e.grad / S)
    pg, pl = dict(g.named_parameters()), dict(gl.named_parameters())
    for w in meta["watch_g"]:
        got["g/grad/" + w] = pg[w].grad.float() / S
    for w in meta["watch_l"]:
        got["gl/grad/" + w] = pl[w].grad.float() / S
    missed = []
    for key, v in got.items():
        v = v.cpu().numpy()
        ref32, ref16 = a["fp32/" + key], a["amp/" + key]
        assert np.isfinite(v).all(), key
        err_ref = np.abs(ref16 - ref32).mean()
        err = np.abs(v - ref32).mean()
        print(f"F17 {key}: mean error to the reference's fp32 result {err:.4e}, the reference's own fp16 run {err_ref:.4e}")
        if not err <= 1.0 * err_ref + 1e-6:
            missed.append((key, err, err_ref))
    assert not missed, missed
    ref_lab = _set_agreement(a["amp/idx"], a["fp32/idx"])
    own_lab = _set_agreement(idx.cpu().numpy(), a["fp32/idx"])
    print(f"F17 label-graph agreement with the fp32 reference: {own_lab:.4f}, the reference's own fp16 run {ref_lab:.4f}")
    assert own_lab >= ref_lab


def test_f17_overflow_surfaces_with_the_switch_on(monkeypatch):
    """An inf planted in the scaled upstream gradient reaches x.grad and a parameter gradient as non-finite through the fp16
    products (nothing clamps or zeroes it); GradScaler skips the step and halves the scale; no parameter changes."""
    from gkgnet_amd import fused
    meta, a, _amp_modules, _, _t = _f17()
    rec, _, _ = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "TRAIN_F16", True)
    g, gl = _amp_modules(meta, a)
    x = _t(a["x"]).requires_grad_(True)
    e = _t(a["e"]).requires_grad_(True)
    params = [p for p in list(g.parameters()) + list(gl.parameters()) if p.requires_grad]
    opt = torch.optim.SGD(params, lr=0.1)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    before = [p.detach().clone() for p in params]
    with torch.autocast("cuda", dtype=F16):
        out = g(x)
        e2, _ = gl(e, out)
    cot = _t(a["cot_x"]).clone()
    cot[0, 0, 0, 0] = float("inf")
    loss = (out.float() * cot).sum() + (e2.float() * _t(a["cot_e"])).sum()
    scaler.scale(loss).backward()
    assert len(rec["f16_dgrad"]) >= 4
    bad = sum(int(not torch.isfinite(p.grad).all()) for p in params if p.grad is not None)
    assert bad > 0 and not torch.isfinite(x.grad).all(), "the overflow must be visible in the gradients"
    scaler.step(opt)                                                 # must skip
    scaler.update()
    assert scaler.get_scale() == 2.0 ** 15
    for p, b in zip(params, before):
        assert torch.equal(p.detach(), b), "GradScaler must skip the step on overflow"
