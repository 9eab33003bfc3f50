#!/usr/bin/env python
"""Neighbour agreement of the two 16-bit contractions (GKG_ENABLE=knn_bf16 / knn_f16) with the index-exact graph at the real stage
shapes — the STAGES table and the structured inputs of tests/test_hip_knn_bf16_real_shapes.py, reduced batch — under bf16 autocast.
Per shape one JSON line: set agreement and mean exact-distance (fp64, relative_pos included) excess of each form against the exact
graph, the number of differing positions, and the share of the nonzero normalised token values the fp16 definition flushes to zero
(fp16 subnormals).  A tool, not a test: the stage-1 shapes take too long for the suite.
    python tools/knn_f16_agreement.py [shape ...]"""
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import test_hip_knn_bf16_real_shapes as S  # noqa: E402
from gkgnet_amd import fused  # noqa: E402
from gkgnet_amd.relpos import build_relative_pos  # noqa: E402


def run(name):
    C, G, H, r, k, d = S.STAGES[name]
    B = 1 if name == "m1" else 2
    gen = torch.Generator(device="cuda").manual_seed(zlib.crc32(name.encode()) % 1000)
    x = S._structured(B, C, H, gen)
    N, c = H * H, C // G
    xt = x.permute(0, 2, 3, 1).reshape(B, N, C).contiguous()
    yt = None if r == 1 else F.avg_pool2d(x, r, r).permute(0, 2, 3, 1).reshape(B, -1, C).contiguous()
    rp = build_relative_pos(C, N, r).cuda()
    graphs = {}
    old = fused.KNN_BF16, fused.KNN_F16
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            for form, (bf, hf) in {"exact": (False, False), "bf16": (True, False), "f16": (False, True)}.items():
                fused.KNN_BF16, fused.KNN_F16 = bf, hf
                graphs[form] = fused.knn_graph_tm(xt, yt, rp, k, d, G)[0]
    finally:
        fused.KNN_BF16, fused.KNN_F16 = old
    xg = F.normalize(xt.view(B, N, G, c).permute(0, 2, 1, 3).reshape(B * G, N, c).double(), dim=-1)
    yg = xg if yt is None else F.normalize(yt.view(B, -1, G, c).permute(0, 2, 1, 3).reshape(B * G, -1, c).double(), dim=-1)
    out = {"shape": name, "C": C, "G": G, "N": N, "M": yg.shape[1], "kd": k * d, "positions": graphs["exact"].numel()}
    e32 = graphs["exact"]
    for form in ("bf16", "f16"):
        e16 = graphs[form]
        exc = 0.0
        for bg in range(B * G):                                               # per problem: (N, M) fp64 stays small
            dist = 2 - 2 * xg[bg] @ yg[bg].t() + rp[0].double()
            exc += (torch.gather(dist, 1, e16[bg]).mean() - torch.gather(dist, 1, e32[bg]).mean()).item()
        out[form + "_set_agreement"] = round((e16.unsqueeze(-1) == e32.unsqueeze(-2)).any(-1).float().mean().item(), 5)
        out[form + "_excess"] = float(f"{exc / (B * G):.3e}")
        out[form + "_differ"] = int((e16 != e32).sum())
    vals = torch.cat([xg.float().flatten()] + ([] if yt is None else [yg.float().flatten()]))
    nz = vals != 0
    out["f16_flushed_share"] = float(f"{((vals.half().abs() < 2.0 ** -14) & nz).sum().item() / max(int(nz.sum()), 1):.3e}")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    os.environ["GKG_RELPOS_DEVICE"] = "cuda"
    for n in (sys.argv[1:] or sorted(S.STAGES)):
        run(n)
