"""GKG_ENABLE=train_grouped at module level: one Grapher + FFN pair in train mode under bf16 / fp16 autocast with gradients (reference
torch_vertex.py:290-333, gkgnet.py:46-72; the grouped layer: BasicConv, torch_nn.py:57-69 behind torch_vertex.py:57-61) — which
launches the grouped projection makes with the add-on switch on and off beside the kind's own switch, what stays bit-identical,
that GKG_DETERMINISTIC keeps the grouped calls and repeats their bits, how close the gradients stay to the fp32 step next to torch's
own mixed precision, that parameter updates reach the stacked fragment arrays, and the F17 fixture's train step and overflow
behaviour with train_f16,train_grouped.

Sizes and helpers: tests/test_hip_train_bf16_modules.py (C 48, G 2, 9 x 9 tokens, B 2 -> 162 rows, k 4; grouped layer 24 -> 24 x 4)."""
import numpy as np
import pytest
import torch

from tests.test_hip_linear_bf16 import _definition
from tests.test_hip_train_bf16_modules import DENSE, _inputs, _pair, _same_bits, _step

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
AMPS = {"bf16": (BF16, "TRAIN_BF16"), "f16": (F16, "TRAIN_F16")}
GROUPED = "g.graph_conv.gconv.nn.0.weight"
GEMMS = ("mm", "addmm", "bmm", "_addmm_activation")


class _GemmProxy:
    """``torch`` as ``fused`` sees it, with the library-GEMM names counted, ``bmm`` among them."""

    def __init__(self, counts):
        self._counts = counts

    def __getattr__(self, name):
        real = getattr(torch, name)
        if name in GEMMS:
            def counted(*a, **k):
                self._counts[name] = self._counts.get(name, 0) + 1
                return real(*a, **k)
            return counted
        return real


def _instrument(monkeypatch):
    """Recording wrappers around the grouped and the dense own callers of ``fused`` (by kind name), the library GEMMs of ``fused``
    counted, and gkg_linear_wgrad_x6's nb recorded."""
    from gkgnet_amd import _lib, fused
    rec, counts, x6 = {"gfwd": [], "gdgrad": [], "fwd": [], "dgrad": []}, {}, []
    for key, name in (("gfwd", "train16_grouped_fwd"), ("gdgrad", "train16_grouped_dgrad"), ("fwd", "train16_fwd"),
                      ("dgrad", "train16_dgrad")):
        def recording(*a, _real=getattr(fused, name), _key=key, **k):
            out = _real(*a, **k)
            rec[_key].append((a[0].name, a[1:], out))
            return out
        monkeypatch.setattr(fused, name, recording)
    lib = _lib.load()
    real_x6 = lib.gkg_linear_wgrad_x6

    def counted(*a):
        x6.append(a[10])                                                         # nb
        return real_x6(*a)
    monkeypatch.setattr(lib, "gkg_linear_wgrad_x6", counted)
    monkeypatch.setattr(fused, "torch", _GemmProxy(counts))
    return rec, counts, x6


def _lens(rec):
    return [len(rec[k]) for k in ("gfwd", "gdgrad", "fwd", "dgrad")]


def _clear(rec, *more):
    for v in list(rec.values()) + list(more):
        v.clear()


def _switches(monkeypatch, kind=None, grouped=False, deterministic=False):
    """Every 16-bit training switch off but ``kind``'s ("bf16" | "f16" | None), the add-on as given."""
    from gkgnet_amd import fused
    monkeypatch.setattr(fused, "TRAIN_BF16", kind == "bf16")
    monkeypatch.setattr(fused, "TRAIN_F16", kind == "f16")
    monkeypatch.setattr(fused, "TRAIN_GROUPED", grouped)
    monkeypatch.setattr(fused, "DETERMINISTIC", deterministic)


@pytest.mark.parametrize("kind", list(AMPS))
def test_dispatch_with_the_add_on_switch_on_and_off(kind, monkeypatch):
    from gkgnet_amd import fused
    assert hasattr(fused, "TRAIN_GROUPED")
    amp = AMPS[kind][0]
    x, cot = _inputs()
    rec, counts, x6 = _instrument(monkeypatch)
    _switches(monkeypatch)
    _step(*_pair(), x, cot, amp=amp)
    assert _lens(rec) == [0, 0, 0, 0]
    all_off = dict(counts)
    _clear(rec, counts, x6)
    _switches(monkeypatch, kind)
    off1 = _step(*_pair(), x, cot, amp=amp)
    kind_only, x6_off = dict(counts), list(x6)
    assert _lens(rec) == [0, 0, 4, 4]
    assert kind_only.get("bmm", 0) == all_off.get("bmm", 0) == 2                  # the grouped forward and input gradient, as today
    assert sum(kind_only.get(n, 0) for n in GEMMS) == 2
    _clear(rec, counts, x6)
    _switches(monkeypatch, kind, grouped=True)
    on = _step(*_pair(), x, cot, amp=amp)
    print(f"{kind}: own launches (grouped fwd, grouped dgrad, dense fwd, dense dgrad) {_lens(rec)}; library GEMMs of fused: all off "
          f"{all_off}, {kind} only {kind_only}, both {dict(counts)}; x6 weight gradients (nb) {kind} only {x6_off}, both {x6}")
    assert _lens(rec) == [1, 1, 4, 4]
    assert all(r[0] == kind for k in rec for r in rec[k])
    assert sum(counts.get(n, 0) for n in GEMMS) == 0                             # no vendor GEMM left in the pair
    assert sorted(x6) == sorted(x6_off) and 4 in x6                              # the weight gradients stay where they were
    if kind == "f16":
        assert sorted(x6) == [1, 1, 1, 1, 4]
    conv = rec["gfwd"][0][1][1]
    assert conv.groups == 4 and rec["gdgrad"][0][1][1] is conv
    assert tuple(rec["gfwd"][0][2].shape) == (4, 162, 24) and tuple(rec["gdgrad"][0][2].shape) == (162, 96)
    for t in (on[0], on[1], *on[2].values()):
        assert bool(torch.isfinite(t).all())
    _clear(rec, counts, x6)
    _switches(monkeypatch, kind)
    off2 = _step(*_pair(), x, cot, amp=amp)
    assert _lens(rec) == [0, 0, 4, 4]
    _same_bits(off1, off2)


@pytest.mark.parametrize("case", ["bf16 without train_bf16", "f16 without train_f16", "bf16 beside train_f16", "f16 beside train_bf16",
                                  "fp32"])
def test_out_of_scope_steps_keep_their_bits(case, monkeypatch):
    """The add-on switch without the kind's own switch (off, or only the OTHER kind's on), and outside autocast: no grouped call, the
    bits of the run with the add-on off."""
    x, cot = _inputs()
    rec, _, _ = _instrument(monkeypatch)
    amp, other = {"bf16 without train_bf16": (BF16, None), "f16 without train_f16": (F16, None), "bf16 beside train_f16": (BF16, "f16"),
                  "f16 beside train_bf16": (F16, "bf16"), "fp32": (None, "f16")}[case]
    got = {}
    for on in (False, True):
        _switches(monkeypatch, other, grouped=on)
        got[on] = _step(*_pair(), x, cot, amp=amp)
        assert _lens(rec) == [0, 0, 0, 0], case
    _same_bits(got[False], got[True])


@pytest.mark.parametrize("kind", list(AMPS))
def test_deterministic_keeps_the_grouped_calls_and_repeats_their_bits(kind, monkeypatch):
    """GKG_DETERMINISTIC refuses train_bf16's dense layers (their weight gradient adds atomically) but not the grouped products."""
    x, cot = _inputs()
    rec, _, _ = _instrument(monkeypatch)
    _switches(monkeypatch, kind, grouped=True, deterministic=True)
    runs = []
    for _ in range(2):
        _clear(rec)
        runs.append(_step(*_pair(), x, cot, amp=AMPS[kind][0]))
        assert _lens(rec) == ([1, 1, 4, 4] if kind == "f16" else [1, 1, 0, 0])
    (o1, d1, g1), (o2, d2, g2) = runs
    assert torch.equal(o1, o2) and torch.equal(d1, d2)
    for name in DENSE + (GROUPED,):
        assert torch.equal(g1[name], g2[name]), name
    for t in (o1, d1, *g1.values()):
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("kind", list(AMPS))
def test_gradients_stay_as_close_to_fp32_as_torch_autocast_does(kind, monkeypatch):
    """Yardstick (test_hip_train_bf16_modules.py's method): torch's own mixed precision — the same modules on the composable path
    (fused.ENABLED = False) under the same autocast dtype.  The fp32 run's neighbour graph is forced into every run, so no near-tie
    flip enters.  For dx, the four dense weights' gradients and the grouped weight's, e = mean|g - g_fp32| / mean|g_fp32|: required
    e(both switches) <= 1.5 e(composable) (the project's factor: test_hip_train_bf16_modules.py, F14); e of the kind's switch alone is
    printed next to it."""
    from gkgnet_amd import fused, ops
    amp = AMPS[kind][0]
    x, cot = _inputs()
    edges = []
    real_tm, real_ops = fused.knn_graph_tm, ops.knn_graph

    def recording(*a, **k):
        e = real_tm(*a, **k)
        edges.append(e)
        return e
    _switches(monkeypatch)
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
    comp = _step(*_pair(), x, cot, amp=amp)
    monkeypatch.setattr(fused, "ENABLED", True)
    rec, _, _ = _instrument(monkeypatch)
    _switches(monkeypatch, kind)
    alone = _step(*_pair(), x, cot, amp=amp)
    assert _lens(rec) == [0, 0, 4, 4]
    _clear(rec)
    _switches(monkeypatch, kind, grouped=True)
    on = _step(*_pair(), x, cot, amp=amp)
    assert _lens(rec) == [1, 1, 4, 4]

    def e(run, name):
        g, r = (run[1], ref[1]) if name == "dx" else (run[2][name], ref[2][name])
        return ((g.double() - r.double()).abs().mean() / r.double().abs().mean()).item()
    names = ("dx",) + DENSE + (GROUPED,)
    for name in names:
        print(f"{kind} {name}: mean|g - g_fp32| / mean|g_fp32|  both switches {e(on, name):.4e}  train_{kind} alone {e(alone, name):.4e}  "
              f"composable autocast {e(comp, name):.4e} (ratio {e(on, name) / e(comp, name):.3f})")
    for name in names:
        assert e(on, name) <= 1.5 * e(comp, name), (name, e(on, name), e(comp, name))


@pytest.mark.parametrize("kind", list(AMPS))
def test_parameter_updates_rebuild_the_grouped_fragments(kind, monkeypatch):
    """Step, optimizer step + mark_parameters_updated, step, optimizer step WITHOUT the mark (the version counters see the in-place
    update), step: each grouped forward streams the fragments of the weights it was called with."""
    from gkgnet_amd import derived, fused, linear_bf16
    amp = AMPS[kind][0]
    row = linear_bf16.KINDS[kind]
    x, cot = _inputs()
    rec, _, _ = _instrument(monkeypatch)
    _switches(monkeypatch, kind, grouped=True)
    g, ffn = _pair()
    params = [p for m in (g, ffn) for p in m.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=0.05)
    conv = g.graph_conv.gconv.nn[0]
    assert conv.groups == 4
    planes, w_at, ys = [], [], []
    for i in range(3):
        _clear(rec)
        w_at.append(conv.weight.detach().clone())
        out, dx, grads = _step(g, ffn, x, cot, amp=amp)
        planes.append((derived.peek(conv, row.gslots[0]), derived.peek(conv, row.gslots[1])))
        assert planes[-1][0] is not None and planes[-1][1] is not None
        ys.append([r for r in rec["gfwd"] if r[1][1] is conv])
        for t in (out, dx, *grads.values()):
            assert bool(torch.isfinite(t).all())
        opt.step()
        if i == 0:
            fused.mark_parameters_updated()
    for i in (1, 2):
        assert not torch.equal(w_at[i - 1], w_at[i])
        assert planes[i][0] is not planes[i - 1][0] and planes[i][1] is not planes[i - 1][1]
        assert not torch.equal(planes[i][0], planes[i - 1][0]) and not torch.equal(planes[i][1], planes[i - 1][1])
        (_, a, Y), = ys[i]
        XM = a[0].detach()
        R, ci = XM.shape[0], XM.shape[1] // 4
        xd = XM.to(row.fragment).double().cpu().view(R, 4, ci)
        holds = {}
        for tag, w in (("current", w_at[i]), ("previous", w_at[i - 1])):
            Wp = fused._kperm_weight(w.view(4, -1, ci)).to(row.fragment).double().cpu()
            ok, worst = True, 0.0
            for q in range(4):
                want, bound = _definition(xd[:, q] @ Wp[q].t(), xd[:, q].abs() @ Wp[q].abs().t(), ci, None, torch.zeros(Wp.shape[1]),
                                          None, 0)
                err = (Y[q].double().cpu() - want).abs()
                ok = ok and bool((err <= bound).all())
                worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
            holds[tag] = ok
            print(f"{kind} grouped forward, step {i}, against the {tag} weights: max err / bound {worst:.3f}")
        assert holds["current"] and not holds["previous"]


# ------------------------------------------------------------------------------------------------ F17 with train_f16,train_grouped
def _f17():
    from tests.test_hip_autocast_trainstep import _amp_modules, _set_agreement, _t
    from tests.util import load_fixture
    meta, a = load_fixture("f17_amp_fp16")
    return meta, a, _amp_modules, _set_agreement, _t


def test_f17_train_step_meets_its_bar_with_both_switches_on(monkeypatch):
    """tests/test_hip_train_f16_modules.py::test_f17_train_step_meets_its_bar_with_the_switch_on's step and bar — every output and
    gradient at least as close to the reference's fp32 result as the reference's own fp16-autocast run (+ 1e-6), label neighbour sets
    agreeing with the fp32 reference at least as well as the reference's fp16 run — with GKG_ENABLE=train_f16,train_grouped, and a
    grouped call recorded for the Grapher and for the GrapherLabel."""
    meta, a, _amp_modules, _set_agreement, _t = _f17()
    assert meta["finite"]
    rec, counts, _ = _instrument(monkeypatch)
    _switches(monkeypatch, "f16", grouped=True)
    g, gl = _amp_modules(meta, a)
    S = meta["loss_scale"]
    x = _t(a["x"]).requires_grad_(True)
    e = _t(a["e"]).requires_grad_(True)
    with torch.autocast("cuda", dtype=F16):
        out = g(x)
        e2, idx = gl(e, out)
    loss = ((out.float() * _t(a["cot_x"])).sum() + (e2.float() * _t(a["cot_e"])).sum()) * S
    loss.backward()
    print(f"F17 own launches (grouped fwd, grouped dgrad, dense fwd, dense dgrad): {_lens(rec)}, library GEMMs of fused: {dict(counts)}")
    assert len(rec["fwd"]) >= 4 and len(rec["dgrad"]) >= 4
    for key in ("gfwd", "gdgrad"):
        convs = [r[1][1] for r in rec[key]]
        assert all(r[0] == "f16" for r in rec[key])
        assert any(c is g.graph_conv.gconv.nn[0] for c in convs), key            # the Grapher's grouped layer
        assert any(c is gl.graph_conv.gconv.nn[0] for c in convs), key           # the GrapherLabel's
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


def test_f17_overflow_surfaces_with_both_switches_on(monkeypatch):
    """An inf planted in the scaled upstream gradient reaches x.grad and a parameter gradient as non-finite through the fp16
    products, the grouped ones among them (nothing clamps or zeroes it); GradScaler skips the step and halves the scale; no
    parameter changes."""
    meta, a, _amp_modules, _, _t = _f17()
    rec, _, _ = _instrument(monkeypatch)
    _switches(monkeypatch, "f16", grouped=True)
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
    assert len(rec["dgrad"]) >= 4 and len(rec["gdgrad"]) >= 2
    bad = sum(int(not torch.isfinite(p.grad).all()) for p in params if p.grad is not None)
    assert bad > 0 and not torch.isfinite(x.grad).all(), "the overflow must be visible in the gradients"
    scaler.step(opt)                                                 # must skip
    scaler.update()
    assert scaler.get_scale() == 2.0 ** 15
    for p, b in zip(params, before):
        assert torch.equal(p.detach(), b), "GradScaler must skip the step on overflow"
