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
move over the layer's algorithmic bytes.    python tools/bench_lin_bf16.py [--out FILE.json] [--reps 15] [--batch 32] [--widths 400,640]

--prep cfg3|cfg5: the Grapher.fc1 leg with the k-NN's token preparation riding on it (gkg_linear_bf16_knn_prep,
GKG_ENABLE=lin_bf16,lin_bf16_prep) at every fc1 shape of GKGNet-576 (cfg3, B 32) or pvig_m at 768 x 768 (cfg5, B 16):

    fused   gkg_linear_bf16_knn_prep, then gkg_knn_fwd_tm16 with GKG_KNN_X_PREPARED (no preparation launch for the queries)
    pair    gkg_linear_bf16,          then gkg_knn_fwd_tm16 (whose first launch is the queries' token_prep)

The k-NN call is part of both sides because the library has no entry point that is the preparation launch alone; fc1_only_us /
fc1_prep_us time the two projection launches without it (their difference is what the last-arriver tail costs, the pair's
difference what the removed launch saves on top).  Same alternation, hipGraph replays and cache sweep as above.

--ffn cfg3|cfg5: an FFN's two projections as ONE launch with the hidden kept on chip (gkg_ffn_bf16, GKG_ENABLE=lin_bf16,ffn_bf16) at
every FFN shape (C -> 4C -> C, residual, fp32 + bf16 out) of GKGNet-576 (cfg3, B 32) or pvig_m at 768 x 768 (cfg5, B 16):

    fused   gkg_ffn_bf16
    pair    gkg_linear_bf16 (GELU, bf16 hidden out), then gkg_linear_bf16 (residual, both outputs) — the same bits

Same alternation, hipGraph replays and cache sweep; shapes outside the fused kernel's envelope report the pair alone.

--tail cfg3|cfg5: the second half of a Grapher as ONE launch with the (T, 2C) matrix kept on chip (gkg_mr_fc2_bf16_nn16,
GKG_ENABLE=lin_bf16,mr_fc2_bf16) at the stage shapes of GKGNet-576 (cfg3, B 32) or pvig_m at 768 x 768 (cfg5, B 16) inside the kernel's
envelope (C <= 192), over the neighbour lists gkg_knn_fwd_tm16 finds for seeded tokens and their pooled keys (the gather's locality
is part of what is measured):

    fused   gkg_mr_fc2_bf16_nn16
    pair    gkg_mr_linear_bf16_nn16 (bf16 (T, 2C) out), then gkg_linear_bf16 (residual, both outputs) — the same bits

Same alternation, hipGraph replays and cache sweep; shapes outside the envelope report the pair alone.

--train: the three products of a dense layer under bf16 autocast WITH gradients (GKG_ENABLE=train_bf16) at the four dense layers of
the four stage shapes of the cfg4 training step (GKGNet-576, B 32), each against what it replaces in ``fused._LinearBNAct``:

    fwd     gkg_linear_bf16_f32a (fp32 x, fp32 Y)            vs  fused._mm_t under autocast (two casts + vendor GEMM + cast back)
    dgrad   gkg_linear_bf16_f32a (fp32 dY, fragments of W^T)  vs  torch.mm(dY, W) in fp32 (autograd runs the backward outside autocast)
    wgrad   gkg_linear_wgrad_bf16 (+ clearing dW)             vs  gkg_linear_wgrad_x6 (+ clearing dW)

Same alternation, hipGraph replays and cache sweep.

--train --amp f16: the two products GKG_ENABLE=train_f16 moves under fp16 autocast, at the same 16 shapes, four legs alternating:

    fwd     gkg_linear_f16_f32a (fp32 x, fp32 Y)             vs  fused._mm_t under fp16 autocast (two casts + vendor GEMM + cast back)
    dgrad   gkg_linear_f16_f32a (fp32 dY, fragments of W^T)   vs  torch.mm(dY, W) in fp32

(the weight gradient keeps its path with that switch).  --amp bf16 is the default: --train alone prints what it always did.

--train --grouped [--amp bf16|f16]: the two products GKG_ENABLE=train_grouped moves beside the kind's own switch, at the GROUPED
projection (Conv2d 2C -> 2C, groups = 4: nb = 4, per-group ci = co = C / 2, XM pitch 2C) of the same four stage shapes:

    fwd     gkg_linear_{bf16,f16}_f32a_grouped (XM in place, Y (4, R, co) fp32)   vs  the autocast torch.bmm on the strided (4, R, ci)
                                                                                     view of XM, its casts and .float() included
    dgrad   gkg_linear_{bf16,f16}_f32a_grouped (dY stacked, dXM written in place)  vs  torch.bmm(dY, W) in fp32 + permute().reshape()

Same alternation, hipGraph replays and cache sweep."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gkgnet_amd import _lib, linear_bf16  # noqa: E402
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


# (C, side of the token grid, side of the pooled key grid) per stage
PREP_CONFIGS = {"cfg3": dict(batch=32, G=2, k=9, stages=((80, 144, 36), (160, 72, 36), (400, 36, 36), (640, 18, 18))),
                "cfg5": dict(batch=16, G=8, k=18, stages=((96, 192, 48), (192, 96, 48), (384, 48, 48), (768, 24, 24)))}


def prep_leg(args, lib, flush):
    cfg = PREP_CONFIGS[args.prep]
    B, G, k, d = (args.batch or cfg["batch"]), cfg["G"], cfg["k"], 1
    rows = []
    for C, side, kside in cfg["stages"]:
        N, M, c, R = side * side, kside * kside, C // G, B * side * side
        has_y = M != N
        gen = torch.Generator(device="cuda").manual_seed(C)
        x = torch.randn(R, C, device="cuda", generator=gen).to(BF16)
        w = torch.randn(C, C, device="cuda", generator=gen) / C ** 0.5
        a = torch.rand(C, device="cuda", generator=gen) + 0.5
        cs = torch.randn(C, device="cuda", generator=gen) * 0.2
        W = torch.zeros((C + 31) // 32 * 32, (C + 15) // 16 * 16, device="cuda", dtype=BF16)
        W[:C, :C] = w.to(BF16)
        planes = W.view(W.shape[0], W.shape[1] // 8, 8).permute(1, 0, 2).contiguous()
        y = torch.randn(B, M, C, device="cuda", generator=gen) if has_y else None
        rp = -torch.rand(N, M, device="cuda", generator=gen)
        flags = _lib.KNN_NORMALIZE | _lib.KNN_RELPOS_UNIT
        if not lib.gkg_linear_bf16_knn_prep_supported(C, B, G, c, N, M, k, d, int(has_y), 1, flags, 0):
            print(f"C={C}: not supported", flush=True)
            continue
        wsb = int(lib.gkg_knn_workspace_bytes(B * G, c, N, M, k, d, _lib.F32, _lib.KNN_NORMALIZE))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        out = torch.empty(R, C, device="cuda")
        nn16 = torch.empty(B * G, N, k, dtype=torch.int16, device="cuda")
        scratch = torch.zeros(int(lib.gkg_linear_bf16_knn_prep_scratch_bytes(R)), dtype=torch.uint8, device="cuda")

        def fc1():
            _lib.check(lib.gkg_linear_bf16(_ptr(x), C, _ptr(planes), _ptr(a), _ptr(cs), None, 0, _ptr(out), C, None, 0, R, C, C, 0,
                                           _stream()), "gkg_linear_bf16")

        def fc1_prep():
            _lib.check(lib.gkg_linear_bf16_knn_prep(_ptr(x), C, _ptr(planes), C, _ptr(a), _ptr(cs), _ptr(out), C, 0, B, G, c, N, M, k, d,
                                                    int(has_y), 1, flags, 0, 0, None, None, _ptr(ws), wsb, _ptr(scratch), scratch.numel(),
                                                    _stream()), "gkg_linear_bf16_knn_prep")

        def knn(prepared):
            _lib.check(lib.gkg_knn_fwd_tm16(_ptr(out), 0, 0, _ptr(y), _ptr(rp), _ptr(nn16), B, G, c, N, M, k, d, _lib.F32,
                                            flags | (_lib.KNN_X_PREPARED if prepared else 0), _ptr(ws), wsb, _stream()), "gkg_knn_fwd_tm16")

        def pair():
            fc1()
            knn(False)

        def fused():
            fc1_prep()
            knn(True)
        pair()
        want = nn16.clone()
        fused()
        torch.cuda.synchronize()
        assert torch.equal(nn16, want) and int(scratch.sum()) == 0               # a sanity check of the comparison, not a test
        graphs = [capture(f) for f in (pair, fused, fc1, fc1_prep)]
        t = [[] for _ in graphs]
        for _ in range(args.reps):                                               # alternate the legs
            for i, g in enumerate(graphs):
                t[i].append(1e3 * replay_ms(g, flush))
        med = [statistics.median(v) for v in t]
        row = dict(config=args.prep, C=C, B=B, G=G, c=c, N=N, M=M, k=k, R=R, pair_us=round(med[0], 1), fused_us=round(med[1], 1),
                   pair_us_min=round(min(t[0]), 1), pair_us_max=round(max(t[0]), 1), fused_us_min=round(min(t[1]), 1),
                   fused_us_max=round(max(t[1]), 1), fc1_only_us=round(med[2], 1), fc1_prep_us=round(med[3], 1),
                   winner="fused" if med[1] < med[0] else "pair")
        rows.append(row)
        print(f"{args.prep} C={C:4d} c={c:3d} N={N:6d} M={M:5d} R={R:7d}: pair {med[0]:8.1f} us [{min(t[0]):.1f}, {max(t[0]):.1f}]  "
              f"fused {med[1]:8.1f} us [{min(t[1]):.1f}, {max(t[1]):.1f}]  fc1 {med[2]:7.1f} us  fc1+prep {med[3]:7.1f} us  -> {row['winner']}",
              flush=True)
        del x, y, rp, ws, out, nn16, graphs
    return rows


def _frag(w16):
    """bf16 weight (cout, cin) -> the fragment array [ci_pad/8][co_pad][8] of gkg_linear_bf16."""
    co, ci = w16.shape
    W = torch.zeros((co + 31) // 32 * 32, (ci + 15) // 16 * 16, device=w16.device, dtype=BF16)
    W[:co, :ci] = w16
    return W.view(W.shape[0], W.shape[1] // 8, 8).permute(1, 0, 2).contiguous()


def ffn_leg(args, lib, flush):
    cfg = PREP_CONFIGS[args.ffn]
    B = args.batch or cfg["batch"]
    rows = []
    for C, side, _ in cfg["stages"]:
        R, H = B * side * side, 4 * C
        gen = torch.Generator(device="cuda").manual_seed(C)
        x = torch.randn(R, C, device="cuda", generator=gen).to(BF16)
        p1 = _frag((torch.randn(H, C, device="cuda", generator=gen) / C ** 0.5).to(BF16))
        p2 = _frag((torch.randn(C, H, device="cuda", generator=gen) / H ** 0.5).to(BF16))
        a1, c1 = torch.rand(H, device="cuda", generator=gen) + 0.5, torch.randn(H, device="cuda", generator=gen) * 0.2
        a2, c2 = torch.rand(C, device="cuda", generator=gen) + 0.5, torch.randn(C, device="cuda", generator=gen) * 0.2
        res = torch.randn(R, C, device="cuda", generator=gen)
        h16 = torch.empty(R, H, device="cuda", dtype=BF16)
        o32, o16 = torch.empty(R, C, device="cuda"), torch.empty(R, C, device="cuda", dtype=BF16)
        f32, f16 = torch.empty(R, C, device="cuda"), torch.empty(R, C, device="cuda", dtype=BF16)

        def pair():
            _lib.check(lib.gkg_linear_bf16(_ptr(x), C, _ptr(p1), _ptr(a1), _ptr(c1), None, 0, None, 0, _ptr(h16), H, R, C, H, 1,
                                           _stream()), "gkg_linear_bf16")
            _lib.check(lib.gkg_linear_bf16(_ptr(h16), H, _ptr(p2), _ptr(a2), _ptr(c2), _ptr(res), C, _ptr(o32), C, _ptr(o16), C, R, H, C,
                                           0, _stream()), "gkg_linear_bf16")

        def fused():
            _lib.check(lib.gkg_ffn_bf16(_ptr(x), C, _ptr(p1), _ptr(a1), _ptr(c1), _ptr(p2), _ptr(a2), _ptr(c2), _ptr(res), C, _ptr(f32), C,
                                        _ptr(f16), C, R, C, H, C, 1, _stream()), "gkg_ffn_bf16")
        # algorithmic bytes: x, both weights, residual, both outputs; the pair moves the hidden twice on top
        ab = R * C * 2 + 2 * C * H * 2 + R * C * (4 + 4 + 2)
        row = dict(config=args.ffn, C=C, hid=H, B=B, R=R, algorithmic_bytes=ab, pair_bytes_ratio=round((ab + 2 * R * H * 2) / ab, 2))
        gp = capture(pair)
        if not lib.gkg_ffn_bf16_supported(R, C, H, C, 1, 1, 1, 1):
            tp = [1e3 * replay_ms(gp, flush) for _ in range(args.reps)]
            row.update(pair_us=round(statistics.median(tp), 1), pair_us_min=round(min(tp), 1), pair_us_max=round(max(tp), 1),
                       fused_us=None, winner="pair (fused: outside the envelope)")
            rows.append(row)
            print(f"{args.ffn} C={C:4d} hid={H:5d} R={R:7d}: pair {row['pair_us']:8.1f} us [{min(tp):.1f}, {max(tp):.1f}]  "
                  f"fused: outside the envelope", flush=True)
            continue
        fused()
        torch.cuda.synchronize()
        assert torch.equal(f32, o32) and torch.equal(f16, o16)                   # a sanity check of the comparison, not a test
        gf = capture(fused)
        tp, tf = [], []
        for _ in range(args.reps):                                               # alternate the legs
            tp.append(1e3 * replay_ms(gp, flush))
            tf.append(1e3 * replay_ms(gf, flush))
        up, uf = statistics.median(tp), statistics.median(tf)
        flop = 4.0 * R * C * H
        row.update(pair_us=round(up, 1), pair_us_min=round(min(tp), 1), pair_us_max=round(max(tp), 1), fused_us=round(uf, 1),
                   fused_us_min=round(min(tf), 1), fused_us_max=round(max(tf), 1), fused_tflops=round(flop / uf * 1e-6, 1),
                   pair_tflops=round(flop / up * 1e-6, 1), fused_GBps=round(ab / uf * 1e-3, 0), winner="fused" if uf < up else "pair")
        rows.append(row)
        print(f"{args.ffn} C={C:4d} hid={H:5d} R={R:7d}: pair {up:8.1f} us [{min(tp):.1f}, {max(tp):.1f}]  "
              f"fused {uf:8.1f} us [{min(tf):.1f}, {max(tf):.1f}] ({row['fused_tflops']:.1f} TFLOP/s, {row['fused_GBps']:.0f} GB/s)"
              f"  -> {row['winner']}", flush=True)
        del x, res, h16, o32, o16, f32, f16, gp, gf
    return rows


def tail_leg(args, lib, flush):
    from gkgnet_amd import derived
    cfg = PREP_CONFIGS[args.tail]
    B, G, k, d = (args.batch or cfg["batch"]), cfg["G"], cfg["k"], 1
    rows = []
    for C, side, kside in cfg["stages"]:
        N, M, c, R = side * side, kside * kside, C // G, B * side * side
        has_y = M != N
        gen = torch.Generator(device="cuda").manual_seed(C)
        x = torch.randn(B, N, C, device="cuda", generator=gen)
        y = None
        if has_y:                                                                # pooled keys, as the block makes them
            r = side // kside
            y = x.view(B, kside, r, kside, r, C).mean(dim=(2, 4)).reshape(B, M, C).contiguous()
        rp = -torch.rand(N, M, device="cuda", generator=gen)
        flags = _lib.KNN_NORMALIZE | _lib.KNN_RELPOS_UNIT
        wsb = int(lib.gkg_knn_workspace_bytes(B * G, c, N, M, k, d, _lib.F32, _lib.KNN_NORMALIZE))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        nn16 = torch.empty(B * G, N, k, dtype=torch.int16, device="cuda")
        _lib.check(lib.gkg_knn_fwd_tm16(_ptr(x), 0, 0, _ptr(y), _ptr(rp), _ptr(nn16), B, G, c, N, M, k, d, _lib.F32, flags, _ptr(ws), wsb,
                                        _stream()), "gkg_knn_fwd_tm16")
        torch.cuda.synchronize()
        del ws, rp
        conv = torch.nn.Conv2d(2 * C, 2 * C, 1, groups=4).cuda()
        p1 = derived.mr_planes(conv)
        p2 = _frag((torch.randn(C, 2 * C, device="cuda", generator=gen) / (2 * C) ** 0.5).to(BF16))
        a1, c1 = torch.rand(2 * C, device="cuda", generator=gen) + 0.5, torch.randn(2 * C, device="cuda", generator=gen) * 0.2
        a2, c2 = torch.rand(C, device="cuda", generator=gen) + 0.5, torch.randn(C, device="cuda", generator=gen) * 0.2
        res = torch.randn(R, C, device="cuda", generator=gen)
        h16 = torch.empty(R, 2 * C, device="cuda", dtype=BF16)
        o32, o16 = torch.empty(R, C, device="cuda"), torch.empty(R, C, device="cuda", dtype=BF16)
        f32, f16 = torch.empty(R, C, device="cuda"), torch.empty(R, C, device="cuda", dtype=BF16)

        def pair():
            _lib.check(lib.gkg_mr_linear_bf16_nn16(_ptr(x), _ptr(y), _ptr(nn16), _ptr(p1), _ptr(a1), _ptr(c1), _ptr(h16), 2 * C, B, G, c,
                                                   N, M, k, 1, _stream()), "gkg_mr_linear_bf16_nn16")
            _lib.check(lib.gkg_linear_bf16(_ptr(h16), 2 * C, _ptr(p2), _ptr(a2), _ptr(c2), _ptr(res), C, _ptr(o32), C, _ptr(o16), C, R,
                                           2 * C, C, 0, _stream()), "gkg_linear_bf16")

        def fused():
            _lib.check(lib.gkg_mr_fc2_bf16_nn16(_ptr(x), _ptr(y), _ptr(nn16), _ptr(p1), _ptr(a1), _ptr(c1), _ptr(p2), _ptr(a2), _ptr(c2),
                                                _ptr(res), C, _ptr(f32), C, _ptr(f16), C, B, G, c, N, M, k, 1, _stream()),
                       "gkg_mr_fc2_bf16_nn16")
        # algorithmic bytes: tokens, keys, lists, both weights, residual, both outputs (a gathered row counted once: the rest is
        # cache traffic); the pair moves the (T, 2C) bf16 matrix twice on top
        ab = R * C * 4 + (B * M * C * 4 if has_y else 0) + B * G * N * k * 2 + C * C * 2 + 2 * C * C * 2 + R * C * (4 + 4 + 2)
        row = dict(config=args.tail, C=C, B=B, G=G, c=c, N=N, M=M, k=k, R=R, algorithmic_bytes=ab,
                   pair_bytes_ratio=round((ab + 2 * R * 2 * C * 2) / ab, 2), fused_bytes_ratio=1.0)
        if not lib.gkg_mr_fc2_bf16_supported(B, G, c, N, M, k, 1, 1, 1, 1):
            gp = capture(pair)
            tp = [1e3 * replay_ms(gp, flush) for _ in range(args.reps)]
            row.update(pair_us=round(statistics.median(tp), 1), pair_us_min=round(min(tp), 1), pair_us_max=round(max(tp), 1),
                       fused_us=None, winner="pair (fused: outside the envelope)")
            rows.append(row)
            print(f"{args.tail} C={C:4d} N={N:6d} M={M:5d} R={R:7d}: pair {row['pair_us']:8.1f} us [{min(tp):.1f}, {max(tp):.1f}]  "
                  f"fused: outside the envelope", flush=True)
            del x, y, res, h16, o32, o16, f32, f16, gp
            continue
        pair()
        fused()
        torch.cuda.synchronize()
        assert torch.equal(f32, o32) and torch.equal(f16, o16)                   # a sanity check of the comparison, not a test
        gp, gf = capture(pair), capture(fused)
        tp, tf = [], []
        for _ in range(args.reps):                                               # alternate the legs
            tp.append(1e3 * replay_ms(gp, flush))
            tf.append(1e3 * replay_ms(gf, flush))
        up, uf = statistics.median(tp), statistics.median(tf)
        row.update(pair_us=round(up, 1), pair_us_min=round(min(tp), 1), pair_us_max=round(max(tp), 1), fused_us=round(uf, 1),
                   fused_us_min=round(min(tf), 1), fused_us_max=round(max(tf), 1), fused_GBps=round(ab / uf * 1e-3, 0),
                   pair_GBps=round(ab / up * 1e-3, 0), winner="fused" if uf < up else "pair")
        rows.append(row)
        print(f"{args.tail} C={C:4d} N={N:6d} M={M:5d} R={R:7d}: pair {up:8.1f} us [{min(tp):.1f}, {max(tp):.1f}] (bytes x{row['pair_bytes_ratio']})  "
              f"fused {uf:8.1f} us [{min(tf):.1f}, {max(tf):.1f}] ({row['fused_GBps']:.0f} GB/s of algorithmic bytes)  -> {row['winner']}",
              flush=True)
        del x, y, res, h16, o32, o16, f32, f16, gp, gf
    return rows


def train_leg(args, lib, flush, kind):
    """--train: the own training products of ``kind`` (a row of linear_bf16.KINDS; --amp) against the paths its switch replaces — the
    forward and the input gradient on the kind's ``*_f32a`` entry point, and the weight gradient where the kind has a kernel of its
    own (bf16; fp16's keeps its path with the switch: nothing to compare)."""
    from gkgnet_amd import derived, fused
    B = args.batch or 32
    widths = {int(t) for t in args.widths.split(",")}
    f32a = getattr(lib, kind.f32a)
    rows = []
    for C, side in ((80, 144), (160, 72), (400, 36), (640, 18)):
        if C not in widths:
            continue
        R = B * side * side
        for name, cin, cout in (("fc1", C, C), ("fc2", 2 * C, C), ("ffn_fc1", C, 4 * C), ("ffn_fc2", 4 * C, C)):
            gen = torch.Generator(device="cuda").manual_seed(cin * 7 + cout)
            conv = torch.nn.Conv2d(cin, cout, 1).cuda()
            x = torch.randn(R, cin, device="cuda", generator=gen)
            dY = torch.randn(R, cout, device="cuda", generator=gen)
            W = conv.weight.detach().view(cout, cin)
            pf, pt = derived.lin_planes(conv, kind), derived.lin_planes(conv, kind, transposed=True)
            Y, dx = torch.empty(R, cout, device="cuda"), torch.empty(R, cin, device="cuda")
            dw_own, dw_x6 = torch.empty(cout, cin, device="cuda"), torch.empty(cout, cin, device="cuda")
            V = {}

            def fwd_own():
                _lib.check(f32a(_ptr(x), cin, _ptr(pf), None, None, None, 0, _ptr(Y), cout, None, 0, R, cin, cout, 0, _stream()), kind.f32a)

            def fwd_old():
                with torch.autocast("cuda", dtype=kind.autocast):
                    V["Y"] = fused._mm_t(x, W)

            def dgrad_own():
                _lib.check(f32a(_ptr(dY), cout, _ptr(pt), None, None, None, 0, _ptr(dx), cin, None, 0, R, cout, cin, 0, _stream()), kind.f32a)

            def dgrad_old():
                V["dx"] = torch.mm(dY, W)

            def wgrad_own():
                dw_own.zero_()
                _lib.check(lib.gkg_linear_wgrad_bf16(_ptr(dY), cout, _ptr(x), cin, _ptr(dw_own), R, cin, cout, _stream()),
                           "gkg_linear_wgrad_bf16")

            def wgrad_old():
                dw_x6.zero_()
                _lib.check(lib.gkg_linear_wgrad_x6(_ptr(dY), cout, 0, _ptr(x), cin, 0, _ptr(dw_x6), R, cin, cout, 1, 0, _stream()),
                           "gkg_linear_wgrad_x6")
            legs = (("fwd", fwd_own, fwd_old), ("dgrad", dgrad_own, dgrad_old), ("wgrad", wgrad_own, wgrad_old))[:3 if kind.own_wgrad else 2]
            graphs = [(capture(a), capture(b)) for _, a, b in legs]
            t = [([], []) for _ in legs]
            for _ in range(args.reps):                                           # alternate all of them
                for i, (ga, gb) in enumerate(graphs):
                    t[i][0].append(1e3 * replay_ms(ga, flush))
                    t[i][1].append(1e3 * replay_ms(gb, flush))
            # the two sides agree to the kind's resolution: a sanity check of the comparison, not a test
            diffs = [(((a - b).abs().max() / b.abs().max()).item()) for a, b in ((Y, V["Y"]), (dx, V["dx"]), (dw_own, dw_x6))[:len(legs)]]
            row = dict(layer=name, C=C, R=R, cin=cin, cout=cout)
            msg = f"C={C:4d} {name:8s} R={R:6d} {cin:4d}->{cout:4d}:"
            for (leg, _, _), (to, tv), d in zip(legs, t, diffs):
                uo, uv = statistics.median(to), statistics.median(tv)
                row.update({f"{leg}_own_us": round(uo, 1), f"{leg}_old_us": round(uv, 1), f"{leg}_own_us_min": round(min(to), 1),
                            f"{leg}_own_us_max": round(max(to), 1), f"{leg}_old_us_min": round(min(tv), 1),
                            f"{leg}_old_us_max": round(max(tv), 1), f"{leg}_own_tflops": round(2.0 * R * cin * cout / uo * 1e-6, 1),
                            f"{leg}_max_rel_diff": float(f"{d:.3e}"), f"{leg}_winner": "own" if uo < uv else "old"})
                msg += f"  {leg} own {uo:7.1f} [{min(to):.1f}, {max(to):.1f}] old {uv:7.1f} [{min(tv):.1f}, {max(tv):.1f}] us"
            rows.append(row)
            print(msg + "  (max rel diff " + " ".join(f"{d:.1e}" for d in diffs) + ")", flush=True)
            del x, dY, Y, dx, V, graphs
    return rows


def grouped_leg(args, lib, flush, kind):
    """--train --grouped: the two products GKG_ENABLE=train_grouped moves (beside the kind's own switch) at the grouped projection of
    the four cfg4 stage shapes (nb = 4, per-group ci = co = C / 2, XM pitch 2C), each against what it replaces in
    ``fused._GroupedLinearBNAct`` on the parent: the autocast bmm on the strided (4, R, ci) view of XM with its casts and .float(), and
    the fp32 bmm + permute().reshape()."""
    from gkgnet_amd import derived, fused
    B = args.batch or 32
    widths = {int(t) for t in args.widths.split(",")}
    rows = []
    for C, side in ((80, 144), (160, 72), (400, 36), (640, 18)):
        if C not in widths:
            continue
        R, nb, ci = B * side * side, 4, C // 2
        co = ci
        gen = torch.Generator(device="cuda").manual_seed(C * 7 + 1)
        conv = torch.nn.Conv2d(2 * C, 2 * C, 1, groups=nb).cuda()
        XM = torch.randn(R, nb * ci, device="cuda", generator=gen)
        dY = torch.randn(nb, R, co, device="cuda", generator=gen)
        Wg = conv.weight.detach().view(nb, co, ci)
        U = XM.view(R, nb, ci).permute(1, 0, 2)
        assert getattr(lib, kind.f32a_grouped_supported)(R, ci, co, nb)
        derived.glin_planes(conv, kind), derived.glin_planes(conv, kind, transposed=True)      # built once, as in a training step
        V = {}

        def fwd_own():
            V["Y_own"] = linear_bf16.train16_grouped_fwd(kind, XM, conv)

        def fwd_old():
            with torch.autocast("cuda", dtype=kind.autocast):
                Y = torch.bmm(U, fused._kperm_weight(Wg).transpose(1, 2))
            V["Y"] = Y.float()

        def dgrad_own():
            V["dXM_own"] = linear_bf16.train16_grouped_dgrad(kind, dY, conv)

        def dgrad_old():
            V["dXM"] = torch.bmm(dY, fused._kperm_weight(Wg)).permute(1, 0, 2).reshape(R, nb * ci)
        legs = (("fwd", fwd_own, fwd_old), ("dgrad", dgrad_own, dgrad_old))
        graphs = [(capture(a), capture(b)) for _, a, b in legs]
        t = [([], []) for _ in legs]
        for _ in range(args.reps):                                               # alternate all of them
            for i, (ga, gb) in enumerate(graphs):
                t[i][0].append(1e3 * replay_ms(ga, flush))
                t[i][1].append(1e3 * replay_ms(gb, flush))
        # the two sides agree to the kind's resolution: a sanity check of the comparison, not a test
        diffs = [((a - b).abs().max() / b.abs().max()).item() for a, b in ((V["Y_own"], V["Y"]), (V["dXM_own"], V["dXM"]))]
        row = dict(layer="grouped", C=C, R=R, nb=nb, ci=ci, co=co, ldxm=nb * ci)
        msg = f"C={C:4d} grouped R={R:6d} {nb} x ({ci:3d}->{co:3d}):"
        for (leg, _, _), (to, tv), d in zip(legs, t, diffs):
            uo, uv = statistics.median(to), statistics.median(tv)
            row.update({f"{leg}_own_us": round(uo, 1), f"{leg}_old_us": round(uv, 1), f"{leg}_own_us_min": round(min(to), 1),
                        f"{leg}_own_us_max": round(max(to), 1), f"{leg}_old_us_min": round(min(tv), 1),
                        f"{leg}_old_us_max": round(max(tv), 1), f"{leg}_own_tflops": round(2.0 * R * nb * ci * co / uo * 1e-6, 1),
                        f"{leg}_own_GBps": round((R * nb * (ci + co) * 4) / uo * 1e-3, 0),
                        f"{leg}_max_rel_diff": float(f"{d:.3e}"), f"{leg}_winner": "own" if uo < uv else "old"})
            msg += f"  {leg} own {uo:7.1f} [{min(to):.1f}, {max(to):.1f}] old {uv:7.1f} [{min(tv):.1f}, {max(tv):.1f}] us -> {row[leg + '_winner']}"
        rows.append(row)
        print(msg + "  (max rel diff " + " ".join(f"{d:.1e}" for d in diffs) + ")", flush=True)
        del XM, dY, V, graphs
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grouped", action="store_true",
                    help="with --train: the grouped projection's forward and input gradient (GKG_ENABLE=train_grouped beside train_bf16 / train_f16) at the cfg4 shapes")
    ap.add_argument("--amp", default="bf16", choices=("bf16", "f16"),
                    help="with --train: the autocast dtype — bf16 (GKG_ENABLE=train_bf16, three products) or f16 (GKG_ENABLE=train_f16: forward and input gradient)")
    ap.add_argument("--train", action="store_true", help="run the three training products (GKG_ENABLE=train_bf16) at the cfg4 shapes")
    ap.add_argument("--prep", default=None, choices=sorted(PREP_CONFIGS), help="run the fc1 + k-NN preparation leg at this config's shapes")
    ap.add_argument("--ffn", default=None, choices=sorted(PREP_CONFIGS), help="run the fused FFN launch against the two-launch pair at this config's shapes")
    ap.add_argument("--tail", default=None, choices=sorted(PREP_CONFIGS), help="run the fused Grapher tail (aggregation + grouped projection + fc2) against the two-launch pair at this config's shapes")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=None, help="default: 32 (cfg3), 16 (--prep cfg5)")
    ap.add_argument("--widths", default="80,160,400,640", help="stage widths C to run (default: all four stages of cfg3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lin_bf16: needs a GPU (a timing anywhere else says nothing)")
    lib = _lib.load()
    flush = torch.empty(128 << 20, dtype=torch.float32, device="cuda")
    if args.train:
        rows = (grouped_leg if args.grouped else train_leg)(args, lib, flush, linear_bf16.KINDS[args.amp])
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(dict(tool="bench_lin_bf16 --train" + (" --grouped --amp " + args.amp if args.grouped else "") +
                               (" --amp f16" if args.amp == "f16" and not args.grouped else ""), batch=args.batch or 32, reps=args.reps,
                               device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
        return
    if args.ffn:
        rows = ffn_leg(args, lib, flush)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(dict(tool="bench_lin_bf16 --ffn", config=args.ffn, reps=args.reps, device=torch.cuda.get_device_name(0),
                               rows=rows), fh, indent=1)
        return
    if args.tail:
        rows = tail_leg(args, lib, flush)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(dict(tool="bench_lin_bf16 --tail", config=args.tail, reps=args.reps, device=torch.cuda.get_device_name(0),
                               rows=rows), fh, indent=1)
        return
    if args.prep:
        rows = prep_leg(args, lib, flush)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(dict(tool="bench_lin_bf16 --prep", config=args.prep, reps=args.reps, device=torch.cuda.get_device_name(0),
                               rows=rows), fh, indent=1)
        return
    args.batch = args.batch or 32
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
            wf = (w * a.view(-1, 1)).to(BF16).contiguous()       # the vendor side's folded weight (derived.folded)
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
