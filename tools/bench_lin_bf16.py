#!/usr/bin/env python
"""Per-layer timing of the own bf16 projection kernel (gkg_linear_bf16, GKG_ENABLE=lin_bf16) against the launches it replaces, at the
four dense projections of a Grapher + FFN pair for every stage of GKGNet-576 (cfg3) at B = 32:

    Grapher.fc1   C -> C    fp32 out                      own  vs  torch.addmm(out_dtype=fp32)          (BN folded into the weight)
    Grapher.fc2   2C -> C   residual, fp32 + bf16 out     own  vs  torch.mm(out_dtype=fp32) + gkg_affine_act_dual
    FFN.fc1       C -> 4C   GELU, bf16 out                own  vs  torch._addmm_activation
    FFN.fc2       4C -> C   residual, fp32 + bf16 out     own  vs  torch.mm(out_dtype=fp32) + gkg_affine_act_dual

Both sides run in the same process, alternating, each replayed from a hipGraph (no launch gaps) with the operands evicted from
the caches by a 512 MB sweep before every replay (in-step conditions, as tools/bench_x6.py); the figure is the median of the
replays.  Reported per layer: microseconds, effective TFLOP/s (2 R cin cout over the time) and the bytes the side's launches
move over the layer's algorithmic bytes.    python tools/bench_lin_bf16.py [--out FILE.json] [--reps 15] [--batch 32] [--widths 400,640]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gkgnet_amd import _lib  # noqa: E402
from gkgnet_amd.ops import _ptr, _stream  # noqa: E402

BF16 = torch.bfloat16


def layer_bytes(R, cin, cout, res, f32, b16):
    """Algorithmic bytes of the fused layer: operands once, results once."""
    return R * cin * 2 + cin * cout * 2 + 8 * cout + (R * cout * 4 if res else 0) + R * cout * ((4 if f32 else 0) + (2 if b16 else 0))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--widths", default="80,160,400,640", help="stage widths C to run (default: all four stages of cfg3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lin_bf16: needs a GPU (a timing anywhere else says nothing)")
    lib = _lib.load()
    flush = torch.empty(128 << 20, dtype=torch.float32, device="cuda")
    rows = []
    widths = {int(t) for t in args.widths.split(",")}
    for C, side in ((80, 144), (160, 72), (400, 36), (640, 18)):
        if C not in widths:
            continue
        R = args.batch * side * side
        for name, cin, cout, act, res, f32, b16 in (("fc1", C, C, 0, False, True, False), ("fc2", 2 * C, C, 0, True, True, True),
                                                    ("ffn_fc1", C, 4 * C, 1, False, False, True),
                                                    ("ffn_fc2", 4 * C, C, 0, True, True, True)):
            gen = torch.Generator(device="cuda").manual_seed(cin * 7 + cout)
            x = torch.randn(R, cin, device="cuda", generator=gen).to(BF16)
            w = (torch.randn(cout, cin, device="cuda", generator=gen) / cin ** 0.5)
            a = torch.rand(cout, device="cuda", generator=gen) + 0.5
            c = torch.randn(cout, device="cuda", generator=gen) * 0.2
            r = torch.randn(R, cout, device="cuda", generator=gen) if res else None
            ci_pad, co_pad = (cin + 15) // 16 * 16, (cout + 31) // 32 * 32
            W = torch.zeros(co_pad, ci_pad, device="cuda", dtype=BF16)
            W[:cout, :cin] = w.to(BF16)
            planes = W.view(co_pad, ci_pad // 8, 8).permute(1, 0, 2).contiguous()
            assert planes.numel() * 2 == lib.gkg_linear_bf16_planes_bytes(cin, cout)
            wf = (w * a.view(-1, 1)).to(BF16).contiguous()       # the vendor side's folded weight (fused._folded_of)
            w16 = w.to(BF16).contiguous()
            o32 = torch.empty(R, cout, device="cuda") if f32 else None
            o16 = torch.empty(R, cout, device="cuda", dtype=BF16) if b16 else None
            v32 = torch.empty(R, cout, device="cuda") if res else None
            v16 = torch.empty(R, cout, device="cuda", dtype=BF16) if res else None
            V = {}                                               # the vendor side's result (the library calls allocate it)
            c16 = c.to(BF16)

            def own():
                _lib.check(lib.gkg_linear_bf16(_ptr(x), cin, _ptr(planes), _ptr(a), _ptr(c), _ptr(r), cout, _ptr(o32), cout, _ptr(o16),
                                               cout, R, cin, cout, act, _stream()), "gkg_linear_bf16")

            if name == "fc1":
                def vendor():
                    V["o"] = torch.addmm(c, x, wf.t(), out_dtype=torch.float32)
                vbytes = layer_bytes(R, cin, cout, False, True, False)
            elif name == "ffn_fc1":
                def vendor():
                    V["o"] = torch._addmm_activation(c16, x, wf.t(), use_gelu=True)
                vbytes = layer_bytes(R, cin, cout, False, False, True)
            else:
                def vendor():
                    y = torch.mm(x, w16.t(), out_dtype=torch.float32)
                    V["o"] = v32
                    _lib.check(lib.gkg_affine_act_dual(_ptr(y), _ptr(a), _ptr(c), _ptr(r), _ptr(v32), _ptr(v16), R, cout, 0, None, 0,
                                                       _stream()), "gkg_affine_act_dual")
                vbytes = layer_bytes(R, cin, cout, False, True, False) + R * cout * 4 + layer_bytes(R, 0, cout, True, True, True)
            go, gv = capture(own), capture(vendor)
            to, tv = [], []
            for _ in range(args.reps):                           # alternate the two sides
                to.append(replay_ms(go, flush))
                tv.append(replay_ms(gv, flush))
            uo, uv = 1e3 * statistics.median(to), 1e3 * statistics.median(tv)
            # same results to bf16 resolution (the folded weight rounds once more): a sanity check of the comparison, not a test
            vo = V["o"].float()
            d = (((o32 if f32 else o16.float()) - vo).abs().max() / vo.abs().max()).item()
            flop = 2.0 * R * cin * cout
            ab = layer_bytes(R, cin, cout, res, f32, b16)
            row = dict(layer=name, C=C, R=R, cin=cin, cout=cout, own_us=round(uo, 1), vendor_us=round(uv, 1),
                       own_tflops=round(flop / uo * 1e-6, 1), vendor_tflops=round(flop / uv * 1e-6, 1),
                       own_us_min=round(1e3 * min(to), 1), vendor_us_min=round(1e3 * min(tv), 1),
                       algorithmic_bytes=ab, own_bytes_ratio=1.0, vendor_bytes_ratio=round(vbytes / ab, 2),
                       own_GBps=round(ab / uo * 1e-3, 0), max_rel_diff=float(f"{d:.3e}"), winner="own" if uo < uv else "vendor")
            rows.append(row)
            print(f"C={C:4d} {name:8s} R={R:6d} {cin:4d}->{cout:4d}: own {uo:8.1f} us ({row['own_tflops']:6.1f} TFLOP/s, "
                  f"{row['own_GBps']:5.0f} GB/s)  vendor {uv:8.1f} us ({row['vendor_tflops']:6.1f} TFLOP/s, bytes x{row['vendor_bytes_ratio']})"
                  f"  -> {row['winner']}  (max rel diff {d:.1e})", flush=True)
            del x, r, o32, o16, v32, v16, V, vo, go, gv
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(tool="bench_lin_bf16", batch=args.batch, reps=args.reps, device=torch.cuda.get_device_name(0), rows=rows),
                      fh, indent=1)


if __name__ == "__main__":
    main()
