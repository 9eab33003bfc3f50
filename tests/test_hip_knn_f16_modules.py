"""GKG_ENABLE=knn_f16 (``fused.KNN_F16``: the fp16-contraction k-NN, GKG_KNN_F16_CONTRACT) at the module level, at ONE small size — the
18 x 18 stage shape C = 80, G = 2, k = 9, d = 1, B = 2 — on the structured inputs of tests/test_hip_knn_bf16_real_shapes.py (``S``) and
the device-built relative_pos.

  graph    under bf16 autocast the fp16 graph differs from the exact one at no more than half as many positions as the bf16 graph
           (operand rounding 2^-12 against 2^-9: a factor 8 expected; host simulation at this size 21-40 against 218-277 of 11 664),
           and the library call carries the fp16 bit and not the bf16 bit;
  block    an eval-mode Grapher under bf16 autocast with each of the three graphs against the product's fp32 run: the fp16 graph
           costs no more than the worse of the other two (+ 2e-3, the additive slack of S's block test);
  scope    the switch acts under fp16 autocast too; outside autocast, and switched off, nothing changes anywhere (bit-identical
           outputs, no flag);
  patched  with ``fused.knn_graph_tm`` patched (a forced graph) the switch changes nothing, as with bf16."""
import contextlib
import os

import pytest
import torch

import test_hip_knn_bf16_real_shapes as S

pytestmark = pytest.mark.gpu

C, G, HW, K, D, B = 80, 2, 18, 9, 1, 2
N = HW * HW
FLAGS_AT = {"gkg_knn_fwd_tm": 15, "gkg_knn_fwd_tm16": 14, "gkg_knn_mr_fwd_tm": 17}      # position of `flags` in the argument lists


@contextlib.contextmanager
def _switches(bf16=False, f16=False):
    from gkgnet_amd import fused
    old = fused.KNN_BF16, fused.KNN_F16
    fused.KNN_BF16, fused.KNN_F16 = bf16, f16
    try:
        yield
    finally:
        fused.KNN_BF16, fused.KNN_F16 = old


@contextlib.contextmanager
def _recorded():
    """-> list of the flag words of the k-NN library calls made inside."""
    from gkgnet_amd import _lib
    lib = _lib.load()
    seen, real = [], {n: getattr(lib, n) for n in FLAGS_AT}

    def wrap(name):
        def f(*a):
            seen.append(int(a[FLAGS_AT[name]]))
            return real[name](*a)
        return f
    for n in FLAGS_AT:
        setattr(lib, n, wrap(n))
    try:
        yield seen
    finally:
        for n in FLAGS_AT:
            setattr(lib, n, real[n])


def _bits(flags):
    from gkgnet_amd import _lib
    return bool(flags & _lib.KNN_BF16_CONTRACT), bool(flags & _lib.KNN_F16_CONTRACT)


def _inputs(seed):
    from gkgnet_amd.relpos import build_relative_pos
    os.environ["GKG_RELPOS_DEVICE"] = "cuda"
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = S._structured(B, C, HW, gen)
    xt = x.permute(0, 2, 3, 1).reshape(B, N, C).contiguous()
    return x, xt, build_relative_pos(C, N, 1).cuda()


def _graph(xt, rp, autocast=torch.bfloat16, **sw):
    from gkgnet_amd import fused
    with _switches(**sw), _recorded() as seen:
        if autocast is None:
            e = fused.knn_graph_tm(xt, None, rp, K, D, G)[0]
        else:
            with torch.autocast("cuda", dtype=autocast):
                e = fused.knn_graph_tm(xt, None, rp, K, D, G)[0]
    assert len(seen) == 1
    return e, _bits(seen[0])


def test_graph_fp16_changes_at_most_half_as_many_neighbours_as_bf16():
    _, xt, rp = _inputs(11)
    exact, fx = _graph(xt, rp)
    e_bf, fb = _graph(xt, rp, bf16=True)
    e_hf, fh = _graph(xt, rp, f16=True)
    assert fx == (False, False) and fb == (True, False) and fh == (False, True), (fx, fb, fh)
    both, fboth = _graph(xt, rp, bf16=True, f16=True)
    assert fboth == (True, False) and torch.equal(both, e_bf), "both switches on: bf16 wins"
    d_bf, d_hf = int((e_bf != exact).sum()), int((e_hf != exact).sum())
    print(f"[knn_f16 graph] positions differing from the exact graph, of {exact.numel()}: bf16 {d_bf}, fp16 {d_hf}")
    assert exact.numel() == 11664 and d_bf > 0
    assert d_hf <= d_bf / 2, (d_hf, d_bf)


def _grapher():
    from gkgnet_amd import layers
    from gkgnet_amd.grapher import Grapher
    from util import keyed_fill_
    os.environ["GKG_RELPOS_DEVICE"] = "cuda"
    layers.norm_cfg["type"] = "BN"
    torch.manual_seed(0)
    mod = Grapher(C, K, D, "mr", "gelu", "batch", True, False, 0.2, 1, n=N, drop_path=0.0, relative_pos=True, use_multi_group=True,
                  num_group=G)
    sd = mod.state_dict()
    keyed_fill_(sd)
    mod.load_state_dict(sd)
    return mod.cuda().eval()


def _run(mod, x, autocast=torch.bfloat16, **sw):
    with _switches(**sw), _recorded() as seen, torch.no_grad():
        if autocast is None:
            out = mod(x)
        else:
            with torch.autocast("cuda", dtype=autocast):
                out = mod(x).float()
    return out, [_bits(f) for f in seen]


def test_block_fp16_graph_is_no_worse_than_the_other_two():
    mod = _grapher()
    x, _, _ = _inputs(7)
    ref, _ = _run(mod, x, autocast=None)                                   # product fp32
    o_exact, f_exact = _run(mod, x)
    o_bf, f_bf = _run(mod, x, bf16=True)
    o_hf, f_hf = _run(mod, x, f16=True)
    assert f_exact == [(False, False)] and f_bf == [(True, False)] and f_hf == [(False, True)], (f_exact, f_bf, f_hf)
    den = (ref - x).norm().item()                                          # the block's own contribution (residual removed)
    e_exact, e_bf, e_hf = ((o - ref).norm().item() / den for o in (o_exact, o_bf, o_hf))
    print(f"[knn_f16 block] rel. error of the graph branch vs product fp32: fp16 contraction {e_hf:.4f}, bf16 contraction {e_bf:.4f}, "
          f"fp32 contraction {e_exact:.4f}")
    assert e_hf <= max(e_bf, e_exact) + 2e-3, (e_hf, e_bf, e_exact)


def test_the_switch_acts_under_autocast_only():
    mod = _grapher()
    x, xt, rp = _inputs(5)
    # fp16 autocast: the switch acts (KNN_BF16 does not: the reference contracts in fp16 there)
    e_hf, f = _graph(xt, rp, autocast=torch.float16, f16=True)
    assert f == (False, True)
    assert _graph(xt, rp, autocast=torch.float16, bf16=True)[1] == (False, False)
    assert torch.equal(_graph(xt, rp, f16=True)[0], e_hf), "the graph does not depend on which 16-bit autocast asked for it"
    # outside autocast the switch changes nothing
    e_off, f_off = _graph(xt, rp, autocast=None)
    e_on, f_on = _graph(xt, rp, autocast=None, f16=True)
    assert f_off == f_on == (False, False) and torch.equal(e_on, e_off)
    assert torch.equal(_graph(xt, rp)[0], e_off), "switched off, autocast callers get the graph fp32 callers get"
    o_off, g_off = _run(mod, x, autocast=None)
    o_on, g_on = _run(mod, x, autocast=None, f16=True)
    assert torch.equal(o_on, o_off) and all(b == (False, False) for b in g_off + g_on)
    # switched off, autocast callers get what they got: the exact graph, the same block output bit for bit
    o_a, g_a = _run(mod, x)
    o_b, g_b = _run(mod, x, f16=False)
    assert torch.equal(o_a, o_b) and g_a == g_b == [(False, False)]
    o_h, g_h = _run(mod, x, autocast=torch.float16, f16=True)
    assert g_h == [(False, True)] and o_h.shape == o_a.shape


def test_a_patched_graph_function_overrides_the_switch():
    from gkgnet_amd import fused
    mod = _grapher()
    x, xt, rp = _inputs(3)
    forced = fused.knn_graph_tm(xt, None, rp, K, D, G).roll(1, dims=2)       # a graph no k-NN form would return
    calls = []

    def forced_graph(*a, **kw):
        calls.append(a)
        return forced
    real = fused.knn_graph_tm
    fused.knn_graph_tm = forced_graph
    try:
        o_off, f_off = _run(mod, x)
        o_on, f_on = _run(mod, x, f16=True)
        o_bf, f_bf = _run(mod, x, bf16=True)
    finally:
        fused.knn_graph_tm = real
    assert len(calls) == 3 and f_off == f_on == f_bf == [], "the forced graph is the only graph"
    assert torch.equal(o_on, o_off) and torch.equal(o_bf, o_off)
