#!/usr/bin/env python
"""Grapher(C=320, 18x18, k=9, G=1) forward + backward in train mode for conv = sage / gin / gat: the HIP aggregation
path against the literal reference form on the same module and inputs (the literal form forced by making the
aggregation module's ``_hip_plan`` return None).  Device-event timing after warm-ups, median of several repeats, and the
peak memory of one step above what the inputs and parameters hold.  One JSON line per (conv, path).

    python tools/bench_gconv.py [--batch 32] [--steps 20] [--warmup 5] [--repeats 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from gkgnet_amd.grapher import Grapher

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--channels", type=int, default=320)
    ap.add_argument("--hw", type=int, default=18)
    ap.add_argument("--k", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--convs", default="sage,gin,gat")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, C, hw = args.batch, args.channels, args.hw
    for conv in args.convs.split(","):
        for path in ("hip", "literal"):
            torch.manual_seed(0)
            mod = Grapher(C, args.k, 1, conv, "gelu", "batch", True, False, 0.2, 1, n=hw * hw, relative_pos=True,
                          use_multi_group=False).to(dev).train()
            gconv = mod.graph_conv.gconv
            if path == "literal":
                gconv._hip_plan = lambda x: None
            x = torch.randn(B, C, hw, hw, device=dev, requires_grad=True)
            g = torch.randn(B, C, hw, hw, device=dev)
            assert (gconv._hip_plan(torch.zeros(1, C, 2, 1, device=dev)) is not None) == (path == "hip")

            def step():
                mod(x).backward(g)

            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.repeats):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.steps):
                    step()
                t1.record()
                torch.cuda.synchronize()
                times.append(t0.elapsed_time(t1) / args.steps)
            x.grad = None
            mod.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            print(json.dumps(dict(conv=conv, path=path, B=B, C=C, hw=hw, k=args.k, ms_fwd_bwd=round(statistics.median(times), 4),
                                  ms_min=round(min(times), 4), ms_max=round(max(times), 4), peak_mib=round(peak / 2**20, 1))),
                  flush=True)
            del mod, x, g
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
