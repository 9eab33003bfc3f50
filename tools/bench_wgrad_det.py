#!/usr/bin/env python
"""Per-layer timing of the run-independent x6 weight gradient (gkg_linear_wgrad_x6_det, GKG_ENABLE=wgrad_det) against the atomic
kernel and against what GKG_DETERMINISTIC=1 runs without the switch, three legs per shape, alternating:

    atomic   gkg_linear_wgrad_x6 into a slot cleared in front of it (the default path)
    det      gkg_linear_wgrad_x6_det, the library's slab rule, the slot as it is
    vendor   fused._wgrad / fused._wgrad_grouped under GKG_DETERMINISTIC without wgrad_det: the vendor (batched) GEMM + sum; for the
             grouped projection's XM operand view also the copy of the operand and the un-permute pass

plus `atomic_noclear` (the atomic launch alone): det minus it is the estimate of what the partial stores and the ordered reduction
add (the library has no entry point that is the reduction alone).  Shapes: the 16 dense layers of the cfg4 training step (GKGNet-576,
B 32: the shapes of tools/bench_lin_bf16.py --train), the grouped projection of each of its stages (nb 4, the XM view with kperm) and
the layers of the cfg2 step (C 320: 10 368 token rows, 2 560 label rows).  Each leg is replayed from a hipGraph with the operands
evicted by a 512 MB sweep before every replay (as tools/bench_lin_bf16.py); reported: median [min, max] of the replays, the slab
count of the det leg.    python tools/bench_wgrad_det.py [--out FILE.json] [--reps 11] [--sets cfg4,cfg4g,cfg2]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gkgnet_amd import _lib, fused  # noqa: E402
from gkgnet_amd.ops import _ptr, _stream  # noqa: E402


def replay_ms(graph, flush):
    flush.add_(1.0)                                               # sweep 512 MB through the caches
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); graph.replay(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def capture(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def shapes(sets):
    out = []
    stages = ((80, 144), (160, 72), (400, 36), (640, 18))
    if "cfg4" in sets:
        for C, side in stages:
            R = 32 * side * side
            out += [(f"cfg4 C={C} {n}", R, ci, co, 1) for n, ci, co in (("fc1", C, C), ("fc2", 2 * C, C), ("ffn_fc1", C, 4 * C),
                                                                        ("ffn_fc2", 4 * C, C))]
    if "cfg4g" in sets:
        out += [(f"cfg4 C={C} grouped", 32 * side * side, C // 2, C // 2, 4) for C, side in stages]
    if "cfg2" in sets:
        for what, R in (("tokens", 10368), ("labels", 2560)):
            out += [(f"cfg2 {what} {n}", R, ci, co, nb) for n, ci, co, nb in (("fc1", 320, 320, 1), ("grouped", 160, 160, 4),
                                                                              ("fc2", 640, 320, 1), ("ffn_fc1", 320, 1280, 1),
                                                                              ("ffn_fc2", 1280, 320, 1))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--sets", default="cfg4,cfg4g,cfg2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wgrad_det: needs a GPU (a timing anywhere else says nothing)")
    lib = _lib.load()
    fused.GEMM_MATH = "x6"
    flush = torch.empty(128 << 20, dtype=torch.float32, device="cuda")
    rows = []
    for name, R, cin, cout, nb in shapes(set(args.sets.split(","))):
        gen = torch.Generator(device="cuda").manual_seed(cin * 7 + cout)
        if nb == 1:
            x = torch.randn(R, cin, device="cuda", generator=gen)
            dY = torch.randn(R, cout, device="cuda", generator=gen)
            ldg, gbs, ldx, xbs, kperm = cout, 0, cin, 0, 0
            xv, shape = x, (cout, cin)
        else:                                                     # the XM operand buffer (R, nb cin) read as (nb, R, cin), kperm
            x = torch.randn(R, nb * cin, device="cuda", generator=gen)
            dY = torch.randn(nb, R, cout, device="cuda", generator=gen)
            ldg, gbs, ldx, xbs, kperm = cout, R * cout, nb * cin, cin, 1
            xv, shape = x.view(R, nb, cin).permute(1, 0, 2), (nb, cout, cin)
        dw_a, dw_d, dw_v = (torch.empty(shape, device="cuda") for _ in range(3))
        ws = torch.empty(int(lib.gkg_linear_wgrad_x6_det_workspace_bytes(R, cin, cout, nb, ldg, ldx, 0)), dtype=torch.uint8, device="cuda")
        slabs = lib.gkg_linear_wgrad_x6_det_slabs(R, cin, cout, nb, ldg, ldx, 1, 0, 0, (ctypes.c_int * 1)(), (ctypes.c_int * 1)(), 0)

        def atomic_noclear():
            _lib.check(lib.gkg_linear_wgrad_x6(_ptr(dY), ldg, gbs, _ptr(x), ldx, xbs, _ptr(dw_a), R, cin, cout, nb, kperm, _stream()),
                       "gkg_linear_wgrad_x6")

        def atomic():
            dw_a.zero_()
            atomic_noclear()

        def det():
            _lib.check(lib.gkg_linear_wgrad_x6_det(_ptr(dY), ldg, gbs, _ptr(x), ldx, xbs, _ptr(dw_d), R, cin, cout, nb, kperm, 0, _ptr(ws),
                                                   ws.numel(), _stream()), "gkg_linear_wgrad_x6_det")

        def vendor():
            fused.DETERMINISTIC, fused.WGRAD_DET = True, False
            try:
                if nb == 1:
                    fused._wgrad(dY, xv, dw_v)
                else:
                    fused._wgrad_grouped(dY, xv, dw_v, kperm=1)
            finally:
                fused.DETERMINISTIC = False
        legs = (("atomic", atomic), ("det", det), ("vendor", vendor), ("atomic_noclear", atomic_noclear))
        graphs = [capture(f) for _, f in legs]
        t = [[] for _ in legs]
        for _ in range(args.reps):                                # alternate the legs
            for i, g in enumerate(graphs):
                t[i].append(1e3 * replay_ms(g, flush))
        atomic()
        torch.cuda.synchronize()
        scale = float(dw_a.abs().max())                           # the three sides agree: a sanity check of the comparison, not a test
        diffs = [float((dw_d - dw_a).abs().max()) / scale, float((dw_v - dw_a).abs().max()) / scale]
        med = [statistics.median(v) for v in t]
        row = dict(layer=name, R=R, cin=cin, cout=cout, nb=nb, det_slabs=int(slabs), partial_MB=round(ws.numel() / 2 ** 20, 2),
                   det_extra_share=round(max(med[1] - med[3], 0.0) / med[1], 3), max_rel_diff_det=float(f"{diffs[0]:.2e}"),
                   max_rel_diff_vendor=float(f"{diffs[1]:.2e}"), det_vs_vendor=round(med[1] / med[2], 3), det_vs_atomic=round(med[1] / med[0], 3))
        msg = f"{name:24s} R={R:7d} {cin:4d}->{cout:4d} nb={nb} slabs={slabs:4d}:"
        for (leg, _), v, m in zip(legs, t, med):
            row.update({f"{leg}_us": round(m, 1), f"{leg}_us_min": round(min(v), 1), f"{leg}_us_max": round(max(v), 1)})
            msg += f"  {leg} {m:8.1f} [{min(v):.1f}, {max(v):.1f}]"
        rows.append(row)
        print(msg + f" us  det/vendor {row['det_vs_vendor']:.2f}  det extra {100 * row['det_extra_share']:.0f} %  "
              f"(diff {diffs[0]:.1e} {diffs[1]:.1e})", flush=True)
        del x, dY, xv, dw_a, dw_d, dw_v, ws, graphs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(tool="bench_wgrad_det", reps=args.reps, device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
