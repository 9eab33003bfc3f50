#!/usr/bin/env python
"""Time the frozen-BatchNorm training step at the cfg2 block pair, and the gkg_bn_eval_bwd kernel on its own.

    python tools/bench_frozen_bn.py --mode frozen            # modules in train(), every BatchNorm in eval(): the fused path
    python tools/bench_frozen_bn.py --mode eval              # whole modules in eval(), gradients on
    python tools/bench_frozen_bn.py --mode train             # train-mode BN (the ordinary step), for scale
    python tools/bench_frozen_bn.py --mode kernel            # gkg_bn_eval_bwd vs bn_bwd_stats + bn_bwd_apply_d, bytes / s
    python tools/bench_frozen_bn.py --mode frozen --bucket --graph    # gradients in a GradBucket; eager, then replayed from a hipGraph

Step: Grapher(C=320, G=4, k=9, d=1, 18x18, relative_pos) -> GrapherLabel(L=80), B=32, fp32, forward + backward of fixed
cotangents, eager launches, device events around all timed steps of a repeat.  ``--root DIR`` imports gkgnet_amd from another
checkout (an older commit timed in the same session: there ``--mode eval`` is the only way through eval-mode BN with gradients,
and it takes the per-op composition).  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="frozen", choices=["frozen", "eval", "train", "kernel"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-fused", action="store_true", help="force the composable path")
    ap.add_argument("--bucket", action="store_true", help="parameter gradients in a parallel.GradBucket (release / pack per step)")
    ap.add_argument("--graph", action="store_true", help="with --bucket: also time the step replayed from a hipGraph (GraphedStep)")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from gkgnet_amd import fused
    if args.no_fused:
        fused.ENABLED = False
    res = kernel_bench(args, torch) if args.mode == "kernel" else step_bench(args, torch, fused)
    res.update(mode=args.mode, label=args.label or os.path.basename(os.path.abspath(args.root)), steps=args.steps, warmup=args.warmup)
    print(json.dumps(res))


def timed(torch, fn, steps, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / steps)
    return out


def step_bench(args, torch, fused):
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    B, C, G, H, k, L = 32, 320, 4, 18, 9, 80
    n = H * H
    torch.manual_seed(0)
    g = Grapher(C, k, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=n, drop_path=0.0, relative_pos=True, use_multi_group=True,
                num_group=G).cuda()
    gl = GrapherLabel(C, k, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=n, drop_path=0.0, relative_pos=False, num_nodes=L,
                      use_multi_group=True, num_group=G).cuda()
    bns = [m for mod in (g, gl) for m in mod.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    with torch.no_grad():
        for m in bns:                                    # non-trivial running statistics
            m.running_mean.normal_(0.0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    train = args.mode != "eval"
    g.train(train)
    gl.train(train)
    if args.mode == "frozen":
        for m in bns:
            m.eval()
    x = torch.randn(B, C, H, H, device="cuda", requires_grad=True)
    e = torch.randn(B, L, C, device="cuda", requires_grad=True)
    cx, ce = torch.randn(B, C, H, H, device="cuda"), torch.randn(B, L, C, device="cuda")
    params = [p for p in list(g.parameters()) + list(gl.parameters()) if p.requires_grad]
    calls = [0]
    real = fused.grapher_forward

    def spy(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)
    fused.grapher_forward = spy

    bucket = None
    if args.bucket:
        from gkgnet_amd import parallel
        bucket = parallel.GradBucket(params)
    drv = [0]
    try:                                                 # calls of the block driver (absent or train-mode only in older checkouts)
        from gkgnet_amd import block
        fwd = block._GrapherBlockFn.forward
        block._GrapherBlockFn.forward = staticmethod(lambda *a: (drv.__setitem__(0, drv[0] + 1), fwd(*a))[1])
    except ImportError:
        pass

    def step():
        if bucket is not None:
            bucket.release(prezero=True)
        else:
            for p in params:
                p.grad = None
        x.grad = e.grad = None
        out = g(x)
        e2, _ = gl(e, out)
        torch.autograd.backward([out, e2], [cx, ce])
        if bucket is not None:
            bucket.pack()
    ms = timed(torch, step, args.steps, args.warmup, args.repeats)
    res = dict(ms_per_step=[round(v, 4) for v in ms], median_ms=round(statistics.median(ms), 4), fused_path=calls[0] > 0,
               block_driver=drv[0] > 0, bias_grad=g.fc1[0].bias.grad is not None, bucket=bucket is not None)
    if args.graph and bucket is not None:
        from gkgnet_amd.graphed import GraphedStep
        gs = GraphedStep(step, warmup=3)
        rp = timed(torch, gs.replay, args.steps, args.warmup, args.repeats)
        res.update(captured=gs.captured, replay_ms_per_step=[round(v, 4) for v in rp], replay_median_ms=round(statistics.median(rp), 4))
    return res


def kernel_bench(args, torch):
    """gkg_bn_eval_bwd (with sums / elementwise only) and the train-mode two-launch backward at the same shapes: achieved
    bytes / s counting one read of dout, one of Y and one write of dY (the train-mode pair reads dout and Y twice)."""
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    lib = _lib.load()
    out = {}
    for name, R, C, nb in (("cfg2_fc", 32 * 324, 320, 1), ("cfg2_grouped", 32 * 324, 160, 4), ("stage1_fc", 32 * 144 * 144, 80, 1)):
        Y, dout, dy = (torch.randn(nb, R, C, device="cuda") for _ in range(3))
        dout2 = dout.permute(1, 0, 2).reshape(R, nb * C).contiguous()            # (R, nb C): row pitch nb C, batch stride C
        gamma, beta, rm = (torch.randn(nb * C, device="cuda") for _ in range(3))
        rv = torch.rand(nb * C, device="cuda") + 0.5
        a, c, mean, invstd, dg, db, dbias = (torch.empty(nb * C, device="cuda") for _ in range(7))
        lib.gkg_bn_eval_affine(_ptr(gamma), _ptr(beta), None, _ptr(rm), _ptr(rv), _ptr(a), _ptr(c), nb * C, 1e-5, _stream())
        mean.copy_(rm)
        invstd.copy_(1.0 / torch.sqrt(rv + 1e-5))
        bufs = torch.zeros(2, 2 * nb * C, dtype=torch.float64, device="cuda")
        state = [0]
        bs = C if nb > 1 else 0

        def eval_sums():
            i = state[0]
            state[0] ^= 1
            _lib.check(lib.gkg_bn_eval_bwd(_ptr(dout2), _ptr(Y), _ptr(a), _ptr(c), _ptr(dy), R, C, nb, nb * C, bs, 1, None, 0, _ptr(rm),
                                           _ptr(rv), None, 1e-5, _ptr(dg), _ptr(db), _ptr(dbias), _ptr(bufs[i]), _ptr(bufs[i ^ 1]),
                                           2 * nb * C, None, 0, _stream()), "gkg_bn_eval_bwd")

        def eval_plain():
            _lib.check(lib.gkg_bn_eval_bwd(_ptr(dout2), _ptr(Y), _ptr(a), _ptr(c), _ptr(dy), R, C, nb, nb * C, bs, 1, None, 0, None,
                                           None, None, 1e-5, None, None, None, None, None, 0, None, 0, _stream()), "gkg_bn_eval_bwd")

        def train_pair():
            i = state[0]
            state[0] ^= 1
            _lib.check(lib.gkg_bn_bwd_atomic(_ptr(dout2), _ptr(Y), _ptr(a), _ptr(c), _ptr(mean), _ptr(invstd), _ptr(dy), _ptr(dg),
                                             _ptr(db), R, C, nb, nb * C, bs, 1, _ptr(bufs[i]), _ptr(bufs[i ^ 1]), 2 * nb * C, _stream()),
                       "gkg_bn_bwd_atomic")
        nbytes = 3.0 * nb * R * C * 4
        for tag, fn in (("eval_bwd_sums", eval_sums), ("eval_bwd_elementwise", eval_plain), ("train_bwd_two_launch", train_pair)):
            bufs.zero_()
            state[0] = 0
            us = [1e3 * v for v in timed(torch, fn, args.steps, args.warmup, args.repeats)]
            out[f"{name}/{tag}"] = dict(us=[round(v, 2) for v in us], tb_per_s=round(nbytes / (statistics.median(us) * 1e-6) / 1e12, 3))
    return out


if __name__ == "__main__":
    main()
