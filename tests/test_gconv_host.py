"""CPU checks of the GraphSAGE / GIN / graph-attention aggregations of GraphConv2d against the reference's fixtures F18-F21
(tools/gen_golden_gconv.py): the modules construct with the reference's state_dict layout and load its checkpoints, and
the aggregation module alone (graph_conv.gconv, the literal torch form on CPU tensors) reproduces the reference's output."""
import numpy as np
import pytest
import torch

from util import load_fixture, state_from

GRAPHER_CASES = ["f18_grapher_sage", "f19_grapher_gin", "f20_grapher_gat"]
LABEL_CASES = ["f21_label_sage_g1", "f21_label_gin_g1", "f21_label_gat_g1"]


def make_grapher(meta):
    from gkgnet_amd.grapher import Grapher
    return Grapher(meta["C"], meta["k"], meta["dilation"], meta["conv"], "gelu", "batch", True, False, 0.2,
                   meta["r"], n=meta["n"], drop_path=0.0, relative_pos=True,
                   use_multi_group=meta["use_multi_group"], num_group=meta["G"])


def make_label(meta):
    from gkgnet_amd.grapher import GrapherLabel
    return GrapherLabel(meta["C"], meta["k"], 1, meta["conv"], "gelu", "batch", True, False, 0.2, 1, n=meta["n"],
                        drop_path=0.0, relative_pos=False, num_nodes=meta["L"],
                        use_multi_group=meta["use_multi_group"], num_group=meta["G"])


def make(meta):
    return make_grapher(meta) if meta["kind"] == "grapher" else make_label(meta)


@pytest.mark.parametrize("name", GRAPHER_CASES + LABEL_CASES)
def test_state_dict_is_checkpoint_compatible(name):
    meta, a = load_fixture(name)
    mod = make(meta)
    ref = state_from(a)
    mine = mod.state_dict()
    assert list(mine.keys()) == list(ref.keys())            # same keys, same order
    for k in ref:
        assert mine[k].shape == ref[k].shape and mine[k].dtype == ref[k].dtype, k
    mod.load_state_dict(ref, strict=True)
    for n, p in mod.named_parameters():
        if "grad/" + n in a:
            assert a["grad/" + n].shape == p.shape, n


def _gconv_inputs(a, suffix):
    x = torch.from_numpy(a["gc_x" + suffix])
    edge = torch.from_numpy(a["gc_edge" + suffix].astype(np.int64))
    y = torch.from_numpy(a["gc_y" + suffix]) if "gc_y" + suffix in a else None
    return x, edge, y


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", GRAPHER_CASES + LABEL_CASES)
def test_literal_gconv_matches_reference_on_cpu(name, train):
    meta, a = load_fixture(name)
    mod = make(meta)
    mod.load_state_dict(state_from(a), strict=True)
    gconv = mod.graph_conv.gconv
    gconv.train(train)
    suffix = "" if train else "_eval"
    x, edge, y = _gconv_inputs(a, suffix)
    assert (y is not None) == (meta["kind"] == "grapher_label" or meta["r"] > 1)
    assert gconv._hip_plan(x) is None                       # CPU tensors: the literal form
    with torch.no_grad():
        out = gconv(x, edge, y)
    want = torch.from_numpy(a["gc_out" + suffix])
    assert out.shape == want.shape
    assert torch.allclose(out, want, atol=1e-5, rtol=1e-5), float((out - want).abs().max())


@pytest.mark.parametrize("name", GRAPHER_CASES)
def test_literal_gconv_backward_runs_on_cpu(name):
    """The literal form is differentiable end to end, eps / a included (the reference's graph on CPU tensors)."""
    meta, a = load_fixture(name)
    mod = make(meta)
    mod.load_state_dict(state_from(a), strict=True)
    x, edge, y = _gconv_inputs(a, "")
    x.requires_grad_(True)
    mod.graph_conv.gconv(x, edge, y).square().sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    for n, p in mod.graph_conv.gconv.named_parameters():
        assert p.grad is not None, n


def test_module_attributes_and_defaults():
    from gkgnet_amd.graph import GINConv2d, GraphAtten, GraphSAGE
    gin = GINConv2d(16, 32, "gelu", "batch")
    assert gin.eps.shape == (1,) and float(gin.eps.detach()) == 0.0 and gin.eps.requires_grad
    assert list(gin.state_dict().keys())[0] == "eps"
    gat = GraphAtten(16, 32, "relu", None, bias=False)
    assert gat.a.in_channels == 32 and gat.a.out_channels == 1 and gat.a.bias is None
    assert isinstance(gat.leakyrelu, torch.nn.LeakyReLU)
    sage = GraphSAGE(16, 32)
    assert sage.nn1[0].in_channels == 16 and sage.nn1[0].out_channels == 16 and sage.nn2[0].in_channels == 32


@pytest.mark.parametrize("conv", ["sage", "gin", "gat"])
def test_dispatch_through_every_wrapper(conv):
    from gkgnet_amd.graph import (DyGraphConv2d, DyGraphConv2dMultiGroup, DyGraphLabel, GINConv2d, GraphAtten,
                                  GraphConv2d, GraphSAGE)
    cls = {"sage": GraphSAGE, "gin": GINConv2d, "gat": GraphAtten}[conv]
    for m in (GraphConv2d(16, 32, conv), DyGraphConv2d(16, 32, 9, 1, conv), DyGraphLabel(16, 32, 9, 1, conv),
              DyGraphConv2dMultiGroup(16, 32, 9, 1, conv, num_head=2)):
        assert isinstance(m.gconv, cls)


def test_unknown_conv_still_raises():
    from gkgnet_amd.graph import GraphConv2d
    with pytest.raises(NotImplementedError, match="conv:bogus is not supported"):
        GraphConv2d(16, 32, conv="bogus")


@pytest.mark.parametrize("conv", ["sage", "gin", "gat"])
def test_multi_group_literal_form_raises_like_the_reference(conv):
    """G > 1 hands the aggregation C/G channels while its convolutions expect C: the reference fails at forward time."""
    from gkgnet_amd.graph import GraphConv2d
    C, G, N, k = 16, 2, 10, 3
    m = GraphConv2d(C, 2 * C, conv, "gelu", "batch")
    x = torch.randn(2 * G, C // G, N, 1)
    idx = torch.randint(0, N, (2 * G, N, k))
    edge = torch.stack([idx, torch.arange(N).view(1, N, 1).expand(2 * G, N, k)])
    with pytest.raises(RuntimeError):
        m(x, edge)
