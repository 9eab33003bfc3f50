#!/usr/bin/env python
"""Golden vectors F18-F21 for the GraphSAGE, GIN and graph-attention aggregations of GraphConv2d, generated FROM THE
REFERENCE ITSELF (torch_vertex.py:16-37 GraphAtten, :116-131 GraphSAGE, :134-150 GINConv2d), like tools/gen_golden.py.

Runs only where the reference tree is (tools/ref_import.py).  Each fixture stores, besides the block-level input / cotangent /
outputs / gradients / state_dict / edge_index of tools/gen_golden.py's Grapher and GrapherLabel cases, the arguments and the
output of ``graph_conv.gconv`` in eval and in train mode (``gc_*`` / ``gc_*_eval``): the tests replay the aggregation module
alone on them, on the CPU (the literal form) as well as on the GPU.

    python tools/gen_golden_gconv.py          # writes tests/golden/f18..f21*.npz
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import np_state, randomize_norm_, ref_top_distances, save  # noqa: E402  (also installs its BN workaround)
from ref_import import load_reference  # noqa: E402


def _gconv_hook(mod, cap, suffix):
    """Records graph_conv.gconv's (x, edge_index, y) and output under gc_*<suffix>."""
    def hook(m, i, o):
        cap["gc_x" + suffix] = i[0].detach().clone()
        cap["gc_edge" + suffix] = i[1].detach().clone()
        if len(i) > 2 and i[2] is not None:
            cap["gc_y" + suffix] = i[2].detach().clone()
        cap["gc_out" + suffix] = o.detach().clone()
    return mod.graph_conv.gconv.register_forward_hook(hook)


def _gconv_arrays(cap):
    out = {}
    for key, v in cap.items():
        if key.startswith("gc_"):
            out[key] = v.numpy().astype(np.int32) if key.startswith("gc_edge") else v.numpy()
    return out


def _grads(mod):
    return {"grad/" + pn: p.grad.numpy() for pn, p in mod.named_parameters() if p.grad is not None}


def grapher_gconv_case(ref, name, *, conv, C, k, d, r, hw, B=2, seed=0):
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed + 1)
    n = hw * hw
    mod = ref.vig.Grapher(C, k, d, conv, "gelu", "batch", True, False, 0.2, r, n=n, drop_path=0.0,
                          relative_pos=True, use_multi_group=False, num_group=1)
    randomize_norm_(mod, gen)
    with torch.no_grad():                    # a non-trivial eps / attention vector (both start at 0 / default init)
        if conv == "gin":
            mod.graph_conv.gconv.eps.fill_(0.3)
    x = torch.randn(B, C, hw, hw, generator=gen)
    cot = torch.randn(B, C, hw, hw, generator=gen)
    sd0 = np_state(mod)

    cap = {}
    h1 = mod.graph_conv.register_forward_hook(lambda m, i, o: cap.update(knn_in=i[0].detach().clone(),
                                                                         edge_index=o[1].detach().clone(),
                                                                         graph=o[0].detach().clone()))
    h2 = _gconv_hook(mod, cap, "_eval")
    mod.eval()
    with torch.no_grad():
        out_eval = mod(x)
    h2.remove()
    eval_edge = cap["edge_index"].clone()
    h2 = _gconv_hook(mod, cap, "")
    mod.train()
    xg = x.clone().requires_grad_(True)
    out = mod(xg)
    (out * cot).sum().backward()
    h1.remove(); h2.remove()

    knn_in = cap["knn_in"]
    xq = knn_in.reshape(B, C, n, 1)
    yk = F.avg_pool2d(knn_in, r, r).reshape(B, C, -1, 1) if r > 1 else None
    topd, topi = ref_top_distances(ref, xq, yk, mod.relative_pos, k * d)
    arrays = dict(x=x.numpy(), cot=cot.numpy(), out_eval=out_eval.numpy(), out=out.detach().numpy(),
                  dx=xg.grad.numpy(), knn_in=knn_in.numpy(), edge_index=cap["edge_index"].numpy().astype(np.int32),
                  edge_index_eval=eval_edge.numpy().astype(np.int32), graph=cap["graph"].numpy(), topd=topd,
                  topi=topi.astype(np.int32))
    arrays.update(_gconv_arrays(cap))
    arrays.update(sd0)
    arrays.update(_grads(mod))
    meta = dict(kind="grapher", C=C, k=k, dilation=d, r=r, n=n, G=1, use_multi_group=False, B=B, hw=hw, conv=conv,
                ref="torch_vertex.py:278-333 + " + {"sage": ":116-131", "gin": ":134-150", "gat": ":16-37"}[conv])
    save(name, meta, **arrays)


def label_gconv_case(ref, name, *, conv, C, k, hw, L, B=2, seed=0):
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed + 1)
    mod = ref.vig.GrapherLabel(C, k, 1, conv, "gelu", "batch", True, False, 0.2, 1, n=hw * hw, drop_path=0.0,
                               relative_pos=False, num_nodes=L, use_multi_group=False, num_group=1)
    randomize_norm_(mod, gen)
    with torch.no_grad():
        if conv == "gin":
            mod.graph_conv.gconv.eps.fill_(-0.2)
    e = torch.randn(B, L, C, generator=gen)
    feat = torch.randn(B, C, hw, hw, generator=gen)
    cot = torch.randn(B, L, C, generator=gen)
    sd0 = np_state(mod)
    cap = {}
    h1 = mod.graph_conv.register_forward_hook(lambda m, i, o: cap.update(knn_in=i[0].detach().clone(),
                                                                         graph=o[0].detach().clone()))
    h2 = _gconv_hook(mod, cap, "_eval")
    mod.eval()
    with torch.no_grad():
        out_eval, idx_eval = mod(e, feat)
    h2.remove()
    h2 = _gconv_hook(mod, cap, "")
    mod.train()
    eg = e.clone().requires_grad_(True)
    fg = feat.clone().requires_grad_(True)
    out, idx = mod(eg, fg)
    (out * cot).sum().backward()
    h1.remove(); h2.remove()
    xq = cap["knn_in"].reshape(B, C, L, 1)
    yk = feat.reshape(B, C, hw * hw, 1)
    topd, topi = ref_top_distances(ref, xq, yk, None, k)
    arrays = dict(e=e.numpy(), feat=feat.numpy(), cot=cot.numpy(), out_eval=out_eval.numpy(),
                  nn_idx_eval=idx_eval.numpy().astype(np.int32), out=out.detach().numpy(),
                  nn_idx=idx.numpy().astype(np.int32), de=eg.grad.numpy(), dfeat=fg.grad.numpy(),
                  knn_in=cap["knn_in"].numpy(), graph=cap["graph"].numpy(), topd=topd, topi=topi.astype(np.int32))
    arrays.update(_gconv_arrays(cap))
    arrays.update(sd0)
    arrays.update(_grads(mod))
    meta = dict(kind="grapher_label", C=C, k=k, n=hw * hw, hw=hw, L=L, G=1, use_multi_group=False, B=B, conv=conv,
                ref="torch_vertex.py:361-403")
    save(name, meta, **arrays)


def main():
    ref = load_reference(with_backbone=False)
    grapher_gconv_case(ref, "f18_grapher_sage", conv="sage", C=32, k=6, d=1, r=2, hw=6, seed=18)
    grapher_gconv_case(ref, "f19_grapher_gin", conv="gin", C=32, k=6, d=2, r=1, hw=6, seed=19)
    grapher_gconv_case(ref, "f20_grapher_gat", conv="gat", C=32, k=6, d=1, r=2, hw=6, seed=20)
    for i, conv in enumerate(("sage", "gin", "gat")):
        label_gconv_case(ref, f"f21_label_{conv}_g1", conv=conv, C=32, k=5, hw=6, L=12, seed=21 + i)


if __name__ == "__main__":
    main()
