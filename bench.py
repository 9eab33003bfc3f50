#!/usr/bin/env python
"""bench.py — Grapher fwd+bwd images/sec on MI355X (BASELINE.json metric).

One "step" = one forward + backward pass of the Group-KNN hot path over one synthetic batch:
    Grapher(C=320, k=9, G=4, d=1, r=1, 18x18, relative_pos)  ->  GrapherLabel(C=320, k=9, G=4, L=80 label tokens)
in train mode (batch-statistics BN), fp32, B=32 images per GPU — BASELINE.json configs[1] ("cfg2-literal").
With N>1 GPUs every rank runs its own B=32 shard (weak scaling) and the step ends with ONE flat RCCL
all-reduce of the parameter gradients.  Inputs are resident in HBM before the timed region.

    python bench.py                       # 1 GPU, default steps
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py --full                # + the other legs, per-kernel timing, rooflines and the CPU baseline
    python bench.py --dump-outputs DIR    # + what the last timed step computed, as DIR/<name>.npy

A plain run only sets up, warms up (cfg2-type workloads: the eager and library-default legs run untimed, as the warm-up the
headline has always followed), times the K steps and prints the headline; everything else it can measure (the figures of
those legs, the per-kernel / roofline figures, the bf16 k-NN leg of cfg3 / cfg5, the CPU baseline) runs with --full.  Prints ONE JSON line on rank 0 (contract: task description / DESIGN.md §Measurement).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (C, G, H, k, d, r, L)
    "cfg2": dict(C=320, G=4, H=18, k=9, d=1, r=1, L=80,
                 desc="BASELINE cfg2-literal: Grapher(C320,G4,k9,d1,18x18,relpos)+GrapherLabel(L80) fwd+bwd"),
    "cfg2ref": dict(C=640, G=2, H=18, k=9, d=3, r=1, L=80,
                    desc="reference stage-4 shape: Grapher(C640,G2,k9,d3,18x18)+GrapherLabel(L80) fwd+bwd"),
    "stage3": dict(C=400, G=2, H=36, k=9, d=2, r=1, L=80,
                   desc="reference stage-3 shape: Grapher(C400,G2,k9,d2,36x36)+GrapherLabel(L80) fwd+bwd"),
    # GKGNet-576 stage 1: 20 736 image tokens x 1 296 pooled keys per image, T = 663 552 rows at B = 32 — the shape where the
    # gather / scatter kernels are genuinely HBM-bandwidth-bound (roofline_hbm)
    "stage1": dict(C=80, G=2, H=144, k=9, d=1, r=4, L=80, cpu_sample=2,
                   desc="reference stage-1 shape: Grapher(C80,G2,k9,d1,r4,144x144,relpos)+GrapherLabel(L80) fwd+bwd"),
}
# whole-backbone workloads (BASELINE.json configs[2..4]): run_backbone()
BACKBONE_WORKLOADS = {
    "cfg3": dict(kind="forward", kw=dict(choice="s", k=9, k_label_gcn=9, n_classes=80, size=576), B=32,
                 desc="BASELINE cfg3: full GKGNet-576 (pvig_s) forward, B=32, bf16 autocast, all 16 graph layers on the HIP kernels"),
    "cfg5": dict(kind="forward", kw=dict(choice="m", k=18, k_label_gcn=18, n_classes=80, size=768, num_group=8), B=16,
                 desc="BASELINE cfg5: pvig_m 768x768 forward, k=18 G=8, B=16, bf16 autocast"),
    "cfg4": dict(kind="train", kw=dict(choice="s", k=9, k_label_gcn=9, n_classes=80, size=576, drop_path=0.1), B=32,
                 desc="BASELINE cfg4: GKGNet-576 training step (ASL x10 + smoothed BCE, AdamW, clip 5.0), fp32, B=32 per GPU, "
                      "data-parallel with RCCL gradient all-reduce"),
}
PEAK_BF16_MFMA_TFLOPS = 2500.0     # dense bf16 matrix peak (no sparsity)
PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: dense fp32 matrix peak (= vector peak)
PEAK_HBM_GBPS = 8000.0
DUMP_BUDGET_BYTES = 60_000_000     # --dump-outputs: all .npy files of one run together stay below 64 MB


def dump_outputs(path, arrays):
    """--dump-outputs: write each tensor of ``arrays`` (name -> tensor) as ``path/<name>.npy``, floating point as float32,
    integer (edge lists) as float64.  When all of them together exceed DUMP_BUDGET_BYTES, every array larger than its
    equal share of the budget is replaced by a fixed sample of its flattened elements: positions drawn without replacement
    by a generator seeded with 0, in ascending order — the same positions in every run with the same arguments."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    items = [(name, t.detach().float() if t.is_floating_point() else t.detach().double()) for name, t in arrays.items()]
    total = sum(t.numel() * t.element_size() for _, t in items)
    share = DUMP_BUDGET_BYTES // max(len(items), 1)
    for name, t in items:
        if total > DUMP_BUDGET_BYTES and t.numel() * t.element_size() > share:
            n = share // t.element_size()
            idx = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))[:n].sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy())
    print(f"[bench] wrote {len(items)} output arrays to {path}" + (" (sampled: larger than the budget)"
                                                                   if total > DUMP_BUDGET_BYTES else ""), file=sys.stderr)


def build_modules(w, device):
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    n = w["H"] * w["H"]
    g = Grapher(w["C"], w["k"], w["d"], "mr", "gelu", "batch", True, False, 0.2, w["r"], n=n, drop_path=0.0,
                relative_pos=True, use_multi_group=True, num_group=w["G"])
    gl = GrapherLabel(w["C"], w["k"], 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=n, drop_path=0.0,
                      relative_pos=False, num_nodes=w["L"], use_multi_group=True, num_group=w["G"])
    return g.to(device).train(), gl.to(device).train()


def cpu_baseline(w, B, grapher, label, x, e, cot_x, cot_e, budget_s=12.0, threads=None):
    """Oracle (torch-CPU restatement of the reference) timed on this box's host cores: the reported baseline.
    ``threads``: torch intra-op threads for this leg (None: torch's default = all cores it is given).  Workloads with a
    ``cpu_sample`` entry time the oracle on that many images of the batch (the reference materialises the (B G, N, M)
    distance tensor: 6.9 GB at stage 1 / B = 32)."""
    sb = min(B, w.get("cpu_sample", B))
    if sb < B:
        x, e, cot_x, cot_e = x[:sb], e[:sb], cot_x[:sb], cot_e[:sb]
        B = sb
    from oracle import torch_ref as R
    old_threads = torch.get_num_threads()
    if threads:
        torch.set_num_threads(threads)
    pg = {k: v.detach().cpu().clone() for k, v in grapher.state_dict().items()}
    pl = {k: v.detach().cpu().clone() for k, v in label.state_dict().items()}
    for d in (pg, pl):
        for k, v in d.items():
            if v.dtype.is_floating_point and "running" not in k and k != "relative_pos":
                v.requires_grad_(True)
    xc, ec = x.detach().cpu().contiguous(), e.detach().cpu()
    cx, ce = cot_x.cpu().contiguous(), cot_e.cpu()

    def step():
        xg, eg = xc.clone().requires_grad_(True), ec.clone().requires_grad_(True)
        out = R.grapher_forward(xg, pg, k=w["k"], dilation=w["d"], r=w["r"], groups=w["G"], training=True)
        e2, _ = R.grapher_label_forward(eg, out, pl, k=w["k"], groups=w["G"], training=True)
        torch.autograd.backward([out, e2], [cx, ce])

    step()                                   # warm-up
    n, t0 = 0, time.perf_counter()
    while True:
        step()
        n += 1
        dt = time.perf_counter() - t0
        if (n >= 3 and dt > budget_s * 0.5) or dt > budget_s or n >= 50:
            break
    used = torch.get_num_threads()
    torch.set_num_threads(old_threads)
    return dict(value=round(B * n / dt, 2), unit="images/s", cores=used, kind="port",
                sample=f"{n} fwd+bwd steps of the same workload (B={B}) on the oracle (oracle/torch_ref.py), "
                       f"{dt:.1f}s, torch CPU fp32, {used} threads; host: {physical_cores()} physical cores / "
                       f"{os.cpu_count()} logical cpus")


def physical_cores() -> int:
    """Physical cores of this host (unique (package, core) pairs in /proc/cpuinfo; SMT siblings counted once)."""
    try:
        pairs, phys, core = set(), None, None
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("physical id"):
                    phys = line.split(":")[1].strip()
                elif line.startswith("core id"):
                    core = line.split(":")[1].strip()
                elif not line.strip():
                    if phys is not None and core is not None:
                        pairs.add((phys, core))
                    phys = core = None
        if phys is not None and core is not None:
            pairs.add((phys, core))
        if pairs:
            return len(pairs)
    except OSError:
        pass
    return os.cpu_count() or 1


def rank_devices(rank, world, local):
    """["rank r: cuda:i (device name)", ...] for every rank of the job (gathered over the process group)."""
    mine = f"rank {rank}: cuda:{local} ({torch.cuda.get_device_name(local)})"
    if world == 1:
        return [mine]
    out = [None] * world
    torch.distributed.all_gather_object(out, mine)
    return out


def spawn_ranks(n: int) -> int:
    """``python bench.py --gpus N`` without a launcher: start N ranks as children (torch.distributed.run, one per GPU,
    rendezvous on 127.0.0.1) BEFORE this process has touched the GPU — it never does: it only relays the children's output
    (rank 0 prints the JSON line) and their exit code.  Mirrors the reference's tools/dist_train.sh:5-7."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def cpu_baseline_backbone(net, head, img, tgt, kind, budget_s=20.0, threads=None):
    """CPU baseline of the whole-backbone workloads: a CPU copy of the same network with the graph operators routed to
    the ORACLE (oracle/torch_ref.py's reference-order k-NN / gather / max; the composable modules around them are plain
    torch — conv2d, batch_norm — exactly what the reference runs: tests/test_backbone.py::
    test_wiring_reproduces_reference_with_oracle_operators pins this arrangement to the reference bit for bit), fp32,
    on a BOUNDED sample of the batch.  ``kind``: "forward" (eval, no_grad) or "train" (forward + loss + backward)."""
    import copy
    import gkgnet_amd.graph as graph
    from oracle import torch_ref as R
    old_threads = torch.get_num_threads()
    if threads:
        torch.set_num_threads(threads)
    real = graph.ops
    graph.ops = type("OracleOps", (), {
        "knn_graph": staticmethod(lambda x, y, rp, k, d: R.knn_graph(x, y, rp, k, d)),
        "max_relative": staticmethod(lambda x, idx, y=None: R.max_relative(x, idx, y))})
    try:
        cnet = copy.deepcopy(net).float().cpu()
        chead = None if head is None else copy.deepcopy(head).float().cpu()
        ci = img.detach().float().cpu()
        ct = None if tgt is None else tgt.detach().float().cpu()

        def step():
            if kind == "forward":
                with torch.no_grad():
                    cnet(ci)
            else:
                cnet.zero_grad(set_to_none=True)
                losses = chead.forward_train(cnet(ci), ct)
                (losses["bce_loss"] + losses["asy_loss"]).backward()
        n, t0 = 0, time.perf_counter()
        while True:
            step()
            n += 1
            dt = time.perf_counter() - t0
            if dt > budget_s * 0.5 or n >= 10:
                break
    finally:
        graph.ops = real
        used = torch.get_num_threads()
        torch.set_num_threads(old_threads)
    b = ci.shape[0]
    return dict(value=round(b * n / dt, 3), unit="images/s", cores=used, kind="port",
                sample=f"{n} {'forward passes' if kind == 'forward' else 'forward + loss + backward passes'} of the same network on "
                       f"{b} image(s) of the batch, graph operators = oracle/torch_ref.py, fp32, {dt:.1f}s, {used} torch threads; "
                       f"host: {physical_cores()} physical cores / {os.cpu_count()} logical cpus")


def run_backbone(args):
    """--workload cfg3 | cfg5 (full-backbone forward, bf16 autocast, eval) and cfg4 (training step, fp32): the same JSON
    schema as the block workloads.  Reference: gkgnet.py:263-284 (forward), label_query_head.py:70-83 + configs/gkgnet/
    gkgnet_coco_576.py:110-126 (loss / optimiser), apis/train.py:117-125 (DDP)."""
    spec = BACKBONE_WORKLOADS[args.workload]
    os.environ.setdefault("GKG_RELPOS_DEVICE", "cuda")
    from gkgnet_amd import _lib, fused, layers, parallel
    from gkgnet_amd.backbone import GKGNet
    rank, world, local = parallel.init_distributed()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    devices = rank_devices(rank, world, local)
    backend = torch.distributed.get_backend() if world > 1 else None
    kind = spec["kind"]
    layers.norm_cfg["type"] = "SyncBN" if (args.sync_bn and world > 1 and kind == "train") else "BN"
    if not args.no_tune:                 # library GEMM selection per shape, tuned during the warm-up passes
        # ... and the library CONVOLUTION selection (the backbone's 3x3 stem / downsample layers run on MIOpen): the
        # reference's own `cudnn_benchmark` config switch (tools/train.py:105-107, tools/test.py:141-143) — MIOpen times its
        # applicable solvers per shape on first use.  cfg3 21.6 -> 19.3 ms, cfg4 86.8 -> 82.5 ms on one box.
        torch.backends.cudnn.benchmark = True
        import torch.cuda.tunable as tunable
        tunable.enable(True)
        tunable.tuning_enable(True)
        tunable.set_max_tuning_duration(30)
        tunable.set_max_tuning_iterations(20 if kind == "forward" else 10)
        tunable.set_filename(os.path.join(os.environ.get("TMPDIR", "/tmp"), f"gkg_tunableop_{args.workload}_rank{rank}.csv"))
    B = args.batch or spec["B"]
    kw = dict(spec["kw"])
    size = kw["size"]
    torch.manual_seed(0)
    t_build = time.perf_counter()
    net = GKGNet(**kw).to(dev)
    build_s = time.perf_counter() - t_build
    gen = torch.Generator().manual_seed(100 + rank)
    img = torch.randn(B, 3, size, size, generator=gen).to(dev)
    steps = args.steps if args.steps is not None else (10 if kind == "forward" else 6)      # default K sized to finish in minutes
    warmup = args.warmup if args.warmup is not None else 3
    head = tgt = None
    n_graph = sum(1 for m in net.modules() if type(m).__name__ in ("Grapher", "GrapherLabel"))

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            el = t.item()
        return el

    def profile(fn, n=2):
        _lib.prof_reset()
        _lib.prof_enable(True)
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        _lib.prof_enable(False)
        prof = _lib.prof_read()
        work = {k: _lib.prof_work(k) / n for k in ("knn_tile", "mr_fwd", "mr_bwd", "gemm_x6")}
        return {k: dict(us_per_step=round(1e3 * v[0] / n, 1), launches_per_step=v[1] // n) for k, v in prof.items() if v[1]}, work

    legs = {}
    last = {}                                # what the last step handed its caller (a captured step: the graph's static outputs)
    if kind == "forward":
        net.eval()

        def fwd():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                out = net(img)
                if args.dump_outputs:
                    last["out"] = out             # no_grad: no autograd graph attached
                return out
        names = ["exact", "bf16"] if args.knn == "both" else [args.knn]
        launch_desc = {}
        for name in names:
            fused.KNN_BF16 = name == "bf16"
            for _ in range(warmup):          # eager warm-up: TunableOp (when on) picks each GEMM shape here, caches fill
                fwd()
            torch.cuda.synchronize()
            # The forward is ~1 300 kernels with static shapes and no host synchronisation: captured once into a hipGraph
            # and replayed (the way a serving loop would run it), the launch gaps between the short kernels disappear.
            step, launch_desc[name] = fwd, "eager (host-launched kernels)"
            if not args.no_graph:
                try:
                    if not args.no_tune:
                        tunable.tuning_enable(False)       # every shape is tuned by now; capture must not time candidates
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        fwd()
                    torch.cuda.current_stream().wait_stream(side)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        out_static = fwd()
                    step, launch_desc[name] = g.replay, "hipGraph replay of the forward"
                except Exception as exc:                   # capture is an optimisation: fall back to eager launches
                    print(f"[bench] hipGraph capture of the forward failed ({type(exc).__name__}: {exc}); running eagerly",
                          file=sys.stderr)
                    torch.cuda.synchronize()
                    fwd()
                    torch.cuda.synchronize()
                finally:
                    if not args.no_tune:
                        tunable.tuning_enable(True)
            el = timed(step)
            if args.dump_outputs and rank == 0 and name == names[0]:
                # the forward's triple: label tokens (B, n_classes, C4), gap (B, C4), the last label graph's edge list
                dump_outputs(args.dump_outputs, {n_: t for n_, t in zip(("label_tokens", "gap", "edge_index"), last["out"])
                                                 if torch.is_tensor(t)})
            kernels, work = profile(fwd) if args.full else (None, None)
            legs[name] = (el, kernels, work)
        fused.KNN_BF16 = names[0] == "bf16"
        headline = names[0]
        launch = launch_desc[headline]
        step_desc = "forward (eval, bf16 autocast)"
        dtype = "bf16"
        metric = "GKGNet forward images/sec"
    else:
        from gkgnet_amd.head import LabelQueryHead, build_optimizer
        net.train()
        head = LabelQueryHead(kw["n_classes"], GKGNet.arch_settings[kw["choice"]]["channels"][-1]).to(dev).train()
        parallel.broadcast_parameters(net)
        parallel.broadcast_parameters(head)
        params = [p for p in list(net.parameters()) + list(head.parameters()) if p.requires_grad]
        bucket = parallel.GradBucket(params)
        opt = build_optimizer([net, head])
        if args.foreach_optimizer:               # A/B: the multi-tensor (foreach) clip + AdamW passes
            opt = torch.optim.AdamW([dict(params=g["params"], weight_decay=g["weight_decay"]) for g in opt.param_groups],
                                    lr=1e-4, betas=(0.9, 0.999), eps=1e-8, fused=False, foreach=True)
        tgt = (torch.rand(B, kw["n_classes"], generator=gen) < 0.04).float().to(dev)
        bucket.install_overlap_hooks()       # chunk all-reduces start during the backward (the reference's DDP reducer)

        def train_step():
            bucket.release(prezero=True)
            losses = head.forward_train(net(img), tgt)
            (losses["bce_loss"] + losses["asy_loss"]).backward()
            if args.dump_outputs:
                last.update({k: v.detach() for k, v in losses.items()})
            bucket.wait()
            if args.foreach_optimizer:
                torch.nn.utils.clip_grad_norm_(params, 5.0)
            else:
                bucket.clip_grad_norm_(5.0)          # the same clipping as a norm + a scale launch on the flat buffer
            opt.step()
        el = timed(train_step)
        if args.dump_outputs and rank == 0:
            # the step's losses, the clipped (all-reduced) gradients it applied and the parameters it left behind
            dump_outputs(args.dump_outputs, dict(bce_loss=last["bce_loss"], asy_loss=last["asy_loss"], param_grads=bucket.flat,
                                                 params=torch.cat([p.detach().reshape(-1) for p in params])))
        kernels, work = profile(train_step, 1) if args.full else (None, None)
        legs["train"] = (el, kernels, work)
        if args.amp != "none":
            # Extra leg: the recipe the reference ships (configs/gkgnet/gkgnet_coco_576.py:146, fp16 AMP with a dynamic loss
            # scale: mmcls/core/fp16/hooks.py) — forward + loss under autocast, scaled backward, unscale, clip, step.
            # The graph kernels, BN statistics and every backward GEMM stay fp32 (tests/test_hip_autocast_trainstep.py, F17).
            amp_dtype = torch.float16 if args.amp == "fp16" else torch.bfloat16
            scaler = torch.amp.GradScaler("cuda", enabled=args.amp == "fp16")

            def amp_step():
                bucket.release(prezero=True)
                with torch.autocast("cuda", dtype=amp_dtype):
                    losses = head.forward_train(net(img), tgt)
                    loss = losses["bce_loss"] + losses["asy_loss"]
                scaler.scale(loss).backward()
                bucket.wait()
                scaler.unscale_(opt)
                bucket.clip_grad_norm_(5.0)
                scaler.step(opt)
                scaler.update()
            legs["amp"] = (timed(amp_step), None, None)
        headline = "train"
        step_desc = "forward + ASL x10 + smoothed BCE + backward + grad all-reduce + clip 5.0 + AdamW"
        dtype = "f32"
        launch = "eager (host-launched kernels)"
        metric = "GKGNet train-step images/sec"

    if rank == 0:
        el, kernels, work = legs[headline]
        kernels, work = kernels or {}, work or {}                    # None: no per-kernel pass (plain run)
        ms_step = 1e3 * el / steps
        value = world * B * steps / el
        roof = None
        if "knn_tile" in kernels and kernels["knn_tile"]["us_per_step"] > 0:
            us = kernels["knn_tile"]["us_per_step"]
            ach = work["knn_tile"] / (us * 1e-6) / 1e12
            peak = PEAK_BF16_MFMA_TFLOPS if headline == "bf16" else PEAK_FP32_MFMA_TFLOPS
            roof = dict(kernel="knn_tile_kernel / knn_pf_kernel (all k-NN launches of the step)", bound="mfma",
                        achieved=round(ach, 2), peak=peak, unit="TFLOP/s", frac=round(ach / peak, 4), traffic=None,
                        us_per_step=us, launches_per_step=kernels["knn_tile"]["launches_per_step"],
                        algorithmic_flops_per_step=work["knn_tile"],
                        note="algorithmic 2 B C N M flop of every graph layer (SURVEY §8d) / summed HIP-event time of the k-NN "
                             "launches; peak: dense fp32 matrix peak for the index-exact contract (the prefilter kernel does the "
                             "bulk on the bf16 cores and may exceed it), dense bf16 peak for the opt-in bf16 contraction")
        roof_hbm = {}
        for name in ("mr_fwd", "mr_bwd"):
            if name in kernels and work.get(name, 0) > 0:
                gbs = work[name] / kernels[name]["us_per_step"] / 1e3
                roof_hbm[name] = dict(bound="hbm", achieved=round(gbs, 1), peak=PEAK_HBM_GBPS, unit="GB/s",
                                      frac=round(gbs / PEAK_HBM_GBPS, 4), algorithmic_bytes_per_step=work[name],
                                      us_per_step=kernels[name]["us_per_step"])
        res = dict(metric=metric, value=round(value, 1), unit="images/s", n_gpus=world, steps=steps, warmup=warmup,
                   ms_per_step=round(ms_step, 3), higher_is_better=True, scaling="weak", vs_baseline=None, dtype=dtype,
                   data="synthetic (random-init weights, N(0,1) images" + (", 4 % positive labels)" if kind == "train" else ")"),
                   config=dict(workload=spec["desc"], step=step_desc, batch_per_gpu=B, global_batch=B * world,
                               input=f"{size}x{size}", graph_layers_on_hip=n_graph, k=kw["k"], groups=kw.get("num_group", 2),
                               bn=("sync" if layers.norm_cfg["type"] == "SyncBN" else "local") if kind == "train" else "eval",
                               parallelism=f"dp{world}", world_size=world, backend=backend or "none (single process)",
                               devices=devices, launch=launch,
                               knn=("index-exact contract (library default; same graphs as fp32)" if headline != "bf16" else
                                    "bf16 contraction (opt-in GKG_KNN_BF16_CONTRACT)"),
                               gemm_selection="library default" if args.no_tune else "TunableOp pass in the warm-up",
                               conv_selection=("library default (immediate mode)" if args.no_tune else
                                               "MIOpen find in the warm-up (cudnn.benchmark, the reference's cudnn_benchmark switch)"),
                               grad_allreduce=("n/a (inference)" if kind == "forward" else
                                               ("none (1 GPU)" if world == 1 else
                                                f"chunked {'RCCL' if backend == 'nccl' else backend} all-reduces started from "
                                                f"post-accumulate hooks during backward"))),
                   peak_mem_GiB=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), model_build_s=round(build_s, 1))
        if args.full:
            res.update(roofline=roof, roofline_hbm=roof_hbm, hip_kernels=kernels)
        if "amp" in legs:
            res[f"ms_per_step_amp_{args.amp}"] = round(1e3 * legs["amp"][0] / steps, 3)
        if kind == "forward":
            for name, (e2, k2, w2) in legs.items():
                res[f"ms_per_step_knn_{name}"] = round(1e3 * e2 / steps, 3)
                if k2 and "knn_tile" in k2:
                    res[f"knn_us_per_step_{name}"] = k2["knn_tile"]["us_per_step"]
        if world == 1 and args.full and not args.no_cpu_baseline:
            sb = 1 if kind == "forward" else 2
            res["cpu_baseline"] = cpu_baseline_backbone(net, head, img[:sb], None if tgt is None else tgt[:sb], kind)
            res["cpu_baseline"]["host_physical_cores"] = physical_cores()
            res["speedup_vs_cpu"] = round(value / max(res["cpu_baseline"]["value"], 1e-9), 1)
        print(json.dumps(res), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: 50; cfg3 / cfg5: 10; cfg4: 6)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed warm-up steps before them (default: 10; cfg3 / cfg4 / cfg5: 3)")
    ap.add_argument("--full", action="store_true",
                    help="also the legs beside the headline (eager launches, library-default GEMM selection, bf16 k-NN for "
                         "cfg3 / cfg5), per-kernel timing and rooflines, and the CPU baseline (unless --no-cpu-baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32 / float64, < 64 MB)")
    ap.add_argument("--workload", default="cfg2", choices=sorted(WORKLOADS) + sorted(BACKBONE_WORKLOADS))
    ap.add_argument("--batch", type=int, default=None, help="images per GPU (default: 32; cfg5: 16)")
    ap.add_argument("--sync-bn", action="store_true", help="SyncBatchNorm across ranks (reference DDP semantics)")
    ap.add_argument("--layout", default="nchw", choices=["nchw", "channels_last"],
                    help="memory format of the feature map and its upstream gradient: nchw (default: what the reference's own "
                         "layers hand to a dropped-in Grapher) or channels_last (what the preceding block of gkgnet_amd's "
                         "backbone hands over: the blocks then chain without layout kernels)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-tune", action="store_true", help="keep the GEMM (and, for the backbone workloads, convolution) libraries' default kernel selection")
    ap.add_argument("--amp", choices=["none", "fp16", "bf16"], default="none",
                    help="cfg4: also time the train step under autocast (fp16 with a dynamic loss scale = the reference's shipped recipe); reported beside the fp32 value")
    ap.add_argument("--foreach-optimizer", action="store_true", help="cfg4: torch's multi-tensor clip_grad_norm_ + foreach AdamW instead of the flat-buffer clip + fused AdamW")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying a hipGraph")
    ap.add_argument("--knn", default=None, choices=["both", "exact", "bf16"],
                    help="cfg3 / cfg5 (bf16 autocast): which k-NN legs to time — exact (the bit-exact index contract, same graphs as "
                         "fp32: the default mode of the library) and / or bf16 (the opt-in GKG_KNN_BF16_CONTRACT contraction); "
                         "default: exact, with --full both")
    args = ap.parse_args()
    if args.knn is None:
        args.knn = "both" if args.full else "exact"

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus))         # no launcher: be the launcher (this process never touches the GPU)
    if args.workload in BACKBONE_WORKLOADS:
        return run_backbone(args)
    if args.batch is None:
        args.batch = 32
    if args.steps is None:
        args.steps = 50
    if args.warmup is None:
        args.warmup = 10
    from gkgnet_amd import _lib, layers, parallel
    rank, world, local = parallel.init_distributed()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    devices = rank_devices(rank, world, local)
    layers.norm_cfg["type"] = "SyncBN" if (args.sync_bn and world > 1) else "BN"
    # --sync-bn: the statistics all-reduces sit inside the step.  Capturing them into the hipGraph is attempted like
    # everything else (RCCL collectives are capturable); if capture fails, or replay loses the untimed vote against eager
    # launches below, the step runs eagerly.
    w = WORKLOADS[args.workload]
    B, C, H, L = args.batch, w["C"], w["H"], w["L"]

    torch.manual_seed(0)
    grapher, label = build_modules(w, dev)
    parallel.broadcast_parameters(grapher)
    parallel.broadcast_parameters(label)
    params = list(grapher.parameters()) + list(label.parameters())
    bucket = parallel.GradBucket(params)

    gen = torch.Generator(device="cpu").manual_seed(1234 + rank)       # every rank its own shard
    x = torch.randn(B, C, H, H, generator=gen).to(dev)
    e = torch.randn(B, L, C, generator=gen).to(dev).requires_grad_(True)
    cot_x = torch.randn(B, C, H, H, generator=gen).to(dev)
    if args.layout == "channels_last":            # same values, (B, H, W, C) memory
        x = x.contiguous(memory_format=torch.channels_last)
        cot_x = cot_x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    cot_e = torch.randn(B, L, C, generator=gen).to(dev)

    def compute():                       # forward + backward + gradient packing: everything on this GPU
        bucket.release(prezero=True)     # ONE fill of the flat gradient buffer instead of a zero-fill per atomically accumulated dW
        x.grad = None
        e.grad = None
        out = grapher(x)
        e2, _ = label(e, out)
        torch.autograd.backward([out, e2], [cot_x, cot_e])
        bucket.pack()
        if args.dump_outputs:                    # what the caller receives (a captured step: the graph's static outputs);
            # detached: holding the outputs themselves keeps this step's autograd graph alive into the next one, whose
            # AccumulateGrad nodes then run on the wrong stream under capture (the process crashed)
            state["out"], state["e2"] = out.detach(), e2.detach()

    def eager_step():
        compute()
        bucket.all_reduce()

    # The step is ~85 short kernels: launched eagerly it is bound by host launch overhead, so the inner loop is
    # captured ONCE into a hipGraph (inputs, weights and the gradient bucket are static buffers) and replayed.
    # host-synchronising collectives (gloo) inside the step cannot be captured: SyncBN all-reduces its statistics in the step
    backend = torch.distributed.get_backend() if world > 1 else None
    capturable = not (world > 1 and args.sync_bn and backend != "nccl")
    if not capturable:
        print("[bench] SyncBN over a non-RCCL backend: the step is launched eagerly", file=sys.stderr)
    # N > 1 over RCCL: the gradient all-reduce is captured INTO the step's hipGraph (RCCL collectives are capturable: the
    # collective becomes a node on RCCL's stream, joined back before the end of the graph) — one graph launch per step, no
    # host-issued collective between replays (reference: the DDP reducer inside backward, mmcls/apis/train.py:117-125).
    # Host-synchronising backends (gloo: the 1-GPU exercise) keep the collective outside the graph.
    state = {"reduce_in_graph": False}

    def measure(steps=None):
        """eager warm-up -> capture -> (multi-rank: replay-vs-eager vote) -> W untimed + K timed steps.  Returns
        (elapsed seconds of the K steps on this rank, captured graph or None)."""
        for _ in range(2):                   # eager warm-up (also where TunableOp, when on, tunes each GEMM shape once)
            compute()
        torch.cuda.synchronize()
        graph = None
        if not args.no_graph and capturable:
            try:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(3):
                        compute()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                if world > 1:
                    torch.distributed.barrier()
                state["reduce_in_graph"] = False
                if world > 1 and backend == "nccl":
                    try:
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g, capture_error_mode="thread_local"):
                            compute()
                            bucket.all_reduce()
                        graph = g
                        state["reduce_in_graph"] = True
                    except Exception as exc:
                        print(f"[bench] capturing the RCCL all-reduce into the step failed ({type(exc).__name__}: {exc}); "
                              f"the collective stays outside the graph", file=sys.stderr)
                        graph = None
                        torch.cuda.synchronize()
                if graph is None:
                    g = torch.cuda.CUDAGraph()
                    # thread_local: RCCL's watchdog thread may poll events while this thread captures
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        compute()
                    graph = g
            except Exception as exc:                       # capture is an optimisation: fall back to eager launches
                print(f"[bench] hipGraph capture failed ({type(exc).__name__}: {exc}); running eagerly", file=sys.stderr)
                graph = None
                torch.cuda.synchronize()
                compute()
                torch.cuda.synchronize()

        def step():
            if graph is None:
                compute()
            else:
                graph.replay()
                if state["reduce_in_graph"]:
                    return
            bucket.all_reduce()

        if graph is not None and world > 1:
            # Multi-rank guard (untimed): replay + collective must actually beat eager launches + collective on this
            # node's runtime; if it does not (the ranks decide together), fall back to eager launches.
            def timed(fn, n=4):
                fn()
                torch.cuda.synchronize()
                torch.distributed.barrier()
                t_ = time.perf_counter()
                for _ in range(n):
                    fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t_) / n
            t_cmp = torch.tensor([timed(step), timed(eager_step)], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t_cmp, op=torch.distributed.ReduceOp.MAX)
            if t_cmp[0].item() > t_cmp[1].item():
                print(f"[bench] hipGraph replay slower than eager launches under this process group "
                      f"({1e3 * t_cmp[0].item():.2f} vs {1e3 * t_cmp[1].item():.2f} ms/step); running eagerly", file=sys.stderr)
                graph = None
                state["reduce_in_graph"] = False

        # untimed: settle clocks / caches / page tables before the W warm-up steps the contract asks for (the first timed leg of
        # a fresh process measured 1-2 % slower than an identical second one without it)
        for _ in range(30 if graph is not None else 3):
            step()
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps or args.steps):
            step()
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            el = t.item()
        return el, graph

    # What a drop-in user inside an eager training loop (the reference's mmcls runner launches every op from Python) gets: the
    # same step without the hipGraph, launched op by op — host launch overhead included.  Reported beside the replayed value.
    # Measured FIRST, in a process that has not captured anything yet: once a hipGraph exists every eager call re-checks the
    # weight planes and clears the BN scratch (a replay may have run in between), which an eager-only user never pays.
    # Every run launches these steps: they are also the untimed eager warm-up (collective included) that the capture and the
    # timed steps below have always followed; the figure itself is reported with --full.
    for _ in range(10):
        eager_step()
    torch.cuda.synchronize()
    n_eager = max(10, min(4 * args.steps, 200))
    t0 = time.perf_counter()
    for _ in range(n_eager):
        eager_step()
    torch.cuda.synchronize()
    ms_eager = 1e3 * (time.perf_counter() - t0) / n_eager

    # Leg 1: the GEMM library's default kernel selection — what a drop-in user gets without a tuning pass (the headline with
    # --no-tune; reported with --full).  A plain run still runs it, at most 200 steps, as the warm-up the headline leg has always
    # followed: without it the headline measured 0.5 % slower on the same box.
    elapsed_no_tune, graph = measure(None if (args.full or args.no_tune) else min(args.steps, 200))
    elapsed = elapsed_no_tune
    if not args.no_tune:
        # Leg 2 (the headline unless --no-tune): the projections that are still plain library GEMMs get PyTorch's
        # TunableOp pick of the fastest rocBLAS / hipBLASLt solution per shape during the (untimed) warm-up.
        import torch.cuda.tunable as tunable
        tunable.enable(True)
        tunable.tuning_enable(True)
        tunable.set_max_tuning_duration(30)
        tunable.set_max_tuning_iterations(40)
        tunable.set_filename(os.path.join(os.environ.get("TMPDIR", "/tmp"), f"gkg_tunableop_rank{rank}.csv"))
        graph = None
        elapsed, graph = measure()

    if args.dump_outputs and rank == 0:          # the last timed step's results, before anything else runs
        dump_outputs(args.dump_outputs, dict(grapher_out=state["out"], label_out=state["e2"], x_grad=x.grad, e_grad=e.grad,
                                             param_grads=bucket.flat))

    from gkgnet_amd import fused
    if args.full:
        # Per-kernel timing for the roofline: the same step, launched eagerly with the library's HIP-event brackets
        # on the launch stream (events cannot bracket individual nodes of a replayed graph).
        prof_steps = max(5, min(args.steps, 20))
        _lib.prof_reset()
        _lib.prof_enable(True)
        for _ in range(prof_steps):
            eager_step()
        torch.cuda.synchronize()
        _lib.prof_enable(False)
        prof = _lib.prof_read()
        # the algorithmic work the library counted for THESE launches (the A/B leg below resets and re-accumulates the counters:
        # reading them later paired one leg's bytes with the other leg's time — VERDICT r5 weak 9)
        prof_work = {name: _lib.prof_work(name) for name in ("mr_fwd", "mr_bwd", "gemm_x6")}

        # the box's own streaming rate (a 256 MiB device-to-device copy: read + write), the practical ceiling of every bandwidth
        # figure below — the pool's boxes differ (4.9-5.5 TB/s measured), 8 TB/s is the data-sheet peak
        cp_src = torch.empty(64 << 20, dtype=torch.float32, device=dev)
        cp_dst = torch.empty_like(cp_src)
        for _ in range(3):
            cp_dst.copy_(cp_src)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(10):
            cp_dst.copy_(cp_src)
        ev1.record()
        torch.cuda.synchronize()
        copy_gbps = 10 * 2 * cp_src.numel() * 4 / (ev0.elapsed_time(ev1) * 1e-3) / 1e9
        del cp_src, cp_dst

        # Row g2 (round 5): by default the k-NN kernel also does the aggregation (fused epilogue), so `knn_tile`'s time below is the
        # fused kernel's and there is no mr_fwd launch.  For continuity with earlier rounds the two-launch form is timed as well.
        prof_two = None
        if fused.KNN_MR:
            fused.KNN_MR = False
            try:
                for _ in range(2):
                    eager_step()
                torch.cuda.synchronize()
                _lib.prof_reset()
                _lib.prof_enable(True)
                for _ in range(prof_steps):
                    eager_step()
                torch.cuda.synchronize()
                _lib.prof_enable(False)
                prof_two = (_lib.prof_read(), _lib.prof_work("mr_fwd") / prof_steps)
            finally:
                fused.KNN_MR = True
    lib_desc = "vendor-library GEMMs (TunableOp-selected)" if not args.no_tune else "vendor-library GEMMs (default heuristic)"
    gemm_desc = {"x6": "fp32 projections: every forward, input-gradient and weight-gradient GEMM on the bf16 matrix cores with an "
                       "exact 3-way operand split, 6 cross products, fp32 accumulation (csrc/gkg_gemm_x6.hip: error vs fp64 below an "
                       "fp32 fma chain's); split-K forms on the label branch's 2 560-row matrices; the weight gradients of the "
                       "backward pass in ONE batched launch; no vendor GEMM in the step",
                 "vendor": lib_desc}[fused.GEMM_MATH]
    if rank == 0:
        ms_step = 1e3 * elapsed / args.steps
        value = world * B * args.steps / elapsed
        res = dict(metric="Grapher fwd+bwd images/sec", value=round(value, 1), unit="images/s", n_gpus=world,
                   steps=args.steps, warmup=args.warmup, ms_per_step=round(ms_step, 4), higher_is_better=True,
                   scaling="weak", vs_baseline=None, dtype="f32", data="synthetic",
                   config=dict(workload=w["desc"], batch_per_gpu=B, global_batch=B * world, C=C, G=w["G"],
                               HW=f"{H}x{H}", k=w["k"], dilation=w["d"], label_tokens=L, bn="sync" if
                               layers.norm_cfg["type"] == "SyncBN" else "local", parallelism=f"dp{world}",
                               input_layout=args.layout,
                               launch="hipGraph replay of fwd+bwd+grad-pack" if graph is not None else "eager",
                               gemm=gemm_desc, world_size=world, backend=backend or "none (single process)",
                               devices=devices,
                               grad_allreduce=("none (1 GPU)" if world == 1 else
                                               f"one flat {'RCCL' if backend == 'nccl' else backend} all-reduce per step, " +
                                               ("captured inside the step's hipGraph" if state["reduce_in_graph"] else
                                                "issued by the host after the replay"))))
        if args.full:
            N = H * H
            M = N // (w["r"] ** 2)
            BG = B * w["G"]
            # algorithmic work of the k-NN tile kernel per step: Grapher graph + label graph
            flops_knn = 2.0 * BG * (C // w["G"]) * (N * M + L * N)
            tile_ms, tile_n = prof["knn_tile"]
            # HBM-side traffic of the same kernel: hardware counters cannot be read from inside the process, so this field is
            # NOT measured by this run — it is the value of the newest committed rocprofv3 --pmc collection for this workload
            # (tools/pmc_refresh.sh -> profiles/rNN_pmc.json), labelled with its file and the commit it was taken at.
            traffic, traffic_source, traffic_by = None, None, {}
            issue_slots = None
            if args.workload == "cfg2" and B == 32:
                import glob
                for pmc_path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc.json")), reverse=True):
                    try:
                        with open(pmc_path) as fh:
                            pj = json.load(fh)
                        # per launch, over the FUSED instantiations on the timed path only (tools/pmc_json.py "knn_mr_fused")
                        traffic = pj["knn_tile_per_step_traffic_bytes"] / pj.get("knn_tile_launches_per_step", 2)
                        traffic_by = {k: v["hbm_bytes_per_launch"] for k, v in pj.get("knn_mr_fused", {}).items()}
                        from gkgnet_amd._build import csrc_sha16
                        same = pj.get("csrc_sha16") == csrc_sha16()
                        if "knn_tile_issue_slot_frac" in pj:
                            issue_slots = dict(issue_slot_frac=pj["knn_tile_issue_slot_frac"], mfma_slot_frac=pj.get("knn_tile_mfma_slot_frac"),
                                               formula="(4 * SQ_INSTS_VALU + SQ_VALU_MFMA_BUSY_CYCLES) / (32 * SQ_BUSY_CYCLES): vector + matrix "
                                                       "issue cycles per SIMD over the launch's busy cycles (same counter collection as `traffic`)")
                        traffic_source = (f"{os.path.relpath(pmc_path, ROOT)} @ {pj.get('commit', '?')} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE "
                                          f"passes, not this run); collected on " +
                                          ("the kernel sources this run uses (csrc hash matches)" if same else
                                           "OTHER kernel sources than this run's (csrc hash differs: stale)"))
                        break
                    except Exception:
                        continue
            roof = None
            if tile_n:
                per_step_ms = tile_ms / prof_steps
                ach = flops_knn / (per_step_ms * 1e-3) / 1e12
                fused_now = prof_two is not None and not prof.get("mr_fwd", (0, 0))[1]
                roof = dict(kernel="knn_tile_kernel<..., MRF> (k-NN + max-relative aggregation in one kernel, row g2)" if fused_now
                            else "knn_tile_kernel", bound="mfma", achieved=round(ach, 2), peak=PEAK_FP32_MFMA_TFLOPS,
                            unit="TFLOP/s", frac=round(ach / PEAK_FP32_MFMA_TFLOPS, 4), traffic=traffic, traffic_source=traffic_source,
                            avg_launch_us=round(1e3 * tile_ms / tile_n, 2), launches_per_step=tile_n // prof_steps,
                            algorithmic_flops_per_step=flops_knn)
                if issue_slots:
                    roof["issue_slots"] = issue_slots
                # the counter traffic next to the ALGORITHMIC bytes of the same launches (SURVEY §8d "Fused fwd (k-NN+MR)": x + (y) +
                # relative_pos + the aggregated output m + the winning rows; no index tensor, no copy of x): ratio > 1 = re-reads
                alg_g = 4.0 * B * C * N + (4.0 * B * C * M if M != N else 0.0) + 4.0 * N * M + 4.0 * B * C * N + 2.0 * B * C * N
                alg_l = 4.0 * B * C * L + 4.0 * B * C * N + 4.0 * B * C * L + 2.0 * B * C * L + 16.0 * BG * L * w["k"]
                roof["algorithmic_bytes_per_launch"] = dict(grapher=alg_g, label=alg_l, mean=(alg_g + alg_l) / 2)
                if traffic_by:
                    roof["traffic_per_launch"] = traffic_by
                    roof["traffic_ratio"] = {k: round(v / dict(grapher=alg_g, label=alg_l)[k], 3) for k, v in traffic_by.items()
                                             if k in ("grapher", "label")}
                    if len(traffic_by) == 2:
                        roof["traffic_ratio"]["step"] = round(sum(traffic_by.values()) / (alg_g + alg_l), 3)
                if fused_now:
                    # SURVEY §8(d) "Fused fwd (k-NN+MR)": the same contraction flop, more bytes — the kernel's time now includes the
                    # gather, so `frac` is NOT comparable with the k-NN-only kernel of rounds 1-4 (0.21-0.23); that kernel, timed
                    # in the two-launch form by this run:
                    t2_ms, t2_n = prof_two[0]["knn_tile"]
                    m2_ms, m2_n = prof_two[0]["mr_fwd"]
                    if t2_n:
                        ach2 = flops_knn / (t2_ms / prof_steps * 1e-3) / 1e12
                        roof["two_launch_form"] = dict(kernel="knn_tile_kernel (k-NN only) + mr_fwd_tm_kernel (GKG_DISABLE=knn_mr)",
                                                       knn_achieved=round(ach2, 2), knn_frac=round(ach2 / PEAK_FP32_MFMA_TFLOPS, 4),
                                                       knn_us_per_step=round(1e3 * t2_ms / prof_steps, 2),
                                                       mr_fwd_us_per_step=round(1e3 * m2_ms / prof_steps, 2),
                                                       mr_fwd_frac_of_hbm=round(prof_two[1] / max(1e3 * m2_ms / prof_steps, 1e-9) / 1e3 / PEAK_HBM_GBPS, 4))
                    roof["note"] = ("frac counts the contraction's flop over the FUSED kernel's whole time (matrix phase + selection + "
                                    "neighbour gather); two_launch_form.knn_frac is the figure comparable with earlier rounds")
            kernels = {k: dict(us_per_step=round(1e3 * v[0] / prof_steps, 2), launches_per_step=v[1] // prof_steps)
                       for k, v in prof.items() if v[1]}
            # HBM-bound companions of the k-NN kernel (the gather + max-relative forward and its scatter backward): ALGORITHMIC
            # bytes per SURVEY §8d, reported by the library per launch (gkg_prof_work), / measured time, vs 8 TB/s
            roof_hbm = {}
            # (round 5: from 160 query rows per image the exact scatter is the one-sweep streaming form; label graphs keep the
            # two-sweep kernel; both are order-independent, so GKG_DETERMINISTIC runs them too)
            mr_bwd_kernel = "mr_bwd_tm_stream_kernel (>= 160 query rows) / mr_bwd_tm_scatter_i64_kernel"
            for name, kern in (("mr_fwd", "mr_fwd_tm_kernel"), ("mr_bwd", mr_bwd_kernel)):
                if name in kernels and kernels[name]["us_per_step"] > 0:
                    nbytes = prof_work[name] / prof_steps
                    gbs = nbytes / kernels[name]["us_per_step"] / 1e3
                    kernels[name].update(bound="hbm", achieved_GBps=round(gbs, 1), frac=round(gbs / PEAK_HBM_GBPS, 4))
                    roof_hbm[name] = dict(kernel=kern, bound="hbm", achieved=round(gbs, 1), peak=PEAK_HBM_GBPS, unit="GB/s",
                                          frac=round(gbs / PEAK_HBM_GBPS, 4), frac_of_copy=round(gbs / copy_gbps, 4),
                                          algorithmic_bytes_per_step=nbytes,
                                          us_per_step=kernels[name]["us_per_step"], launches_per_step=kernels[name]["launches_per_step"])
            if roof is not None and "two_launch_form" in roof:
                # the fused kernel against the HBM roofline with §8(d)'s "Fused fwd (k-NN+MR)" bytes per graph:
                # x + (y) + relative_pos + index lists + the aggregated output
                e4 = 4.0
                by_g, by_l = roof["algorithmic_bytes_per_launch"]["grapher"], roof["algorithmic_bytes_per_launch"]["label"]
                us = kernels["knn_tile"]["us_per_step"]
                gbs = (by_g + by_l) / us / 1e3
                roof_hbm["knn_mr_fused"] = dict(kernel="knn_tile_kernel<..., MRF>", bound="hbm", achieved=round(gbs, 1), peak=PEAK_HBM_GBPS,
                                                unit="GB/s", frac=round(gbs / PEAK_HBM_GBPS, 4), frac_of_copy=round(gbs / copy_gbps, 4),
                                                algorithmic_bytes_per_step=by_g + by_l,
                                                us_per_step=us, launches_per_step=kernels["knn_tile"]["launches_per_step"],
                                                note="compute-bound kernel (SURVEY §8d: 3.7 us at 8 TB/s vs 13.7 us at the fp32 matrix peak for the Grapher graph)")
            if "gemm_x6" in kernels and kernels["gemm_x6"]["us_per_step"] > 0:
                # the projection GEMMs that run on the split-bf16 kernels: algorithmic fp32 flop (2 R cin cout, reported by the
                # library per launch) per second, against the fp32-MFMA peak they replace and against their own bound — six
                # bf16 MFMAs per fp32 block product at the dense bf16 peak (2.5 PFLOP/s / 6)
                gf = prof_work["gemm_x6"] / prof_steps
                tf = gf / kernels["gemm_x6"]["us_per_step"] / 1e6
                kernels["gemm_x6"].update(bound="mfma", algorithmic_flops_per_step=gf, achieved_TFLOPs=round(tf, 1),
                                          frac_of_fp32_mfma_peak=round(tf / PEAK_FP32_MFMA_TFLOPS, 4),
                                          frac_of_split_bf16_bound=round(tf / (2500.0 / 6), 4))
            # Step-level roofline: every algorithmic flop of the step (the projections' forward + input-gradient +
            # weight-gradient GEMMs = 3x their forward, plus the two distance contractions) against the dense fp32 matrix peak,
            # and the bytes that must cross HBM at least once (inputs, cotangents, input gradients, weights and weight
            # gradients, relative_pos, the edge lists) against 8 TB/s.  The larger of the two times bounds the step.
            T, TL = B * N, B * L
            flops_proj = 3.0 * (8.0 * T * C * C + 24.0 * TL * C * C)
            flops_step = flops_proj + flops_knn
            n_par = sum(p.numel() for p in params)
            bytes_step = 4.0 * (3 * B * C * N + 3 * B * L * C + B * C * N) + 8.0 * n_par + 4.0 * N * M + 8.0 * BG * (N + L) * w["k"]
            t_flop = flops_step / (PEAK_FP32_MFMA_TFLOPS * 1e12)
            t_byte = bytes_step / (PEAK_HBM_GBPS * 1e9)
            roof_step = dict(bound="mfma" if t_flop >= t_byte else "hbm", algorithmic_flops=flops_step,
                             algorithmic_bytes=bytes_step, flop_time_ms_at_fp32_peak=round(1e3 * t_flop, 4),
                             byte_time_ms_at_8TBps=round(1e3 * t_byte, 4), achieved_TFLOPs=round(flops_step / (ms_step * 1e-3) / 1e12, 2),
                             peak=PEAK_FP32_MFMA_TFLOPS, frac=round(max(t_flop, t_byte) / (ms_step * 1e-3), 4),
                             note="projections 3 x (8 T C^2 + 24 T_L C^2) + k-NN 2 B C (N M + L N) flop; fp32 matrix peak "
                                  "(the split-bf16 kernels may exceed it: their own bound is the bf16 peak / 6)")
            res.update(roofline=roof, roofline_hbm=roof_hbm, roofline_step=roof_step, hip_kernels=kernels,
                       hbm_copy_GBps=round(copy_gbps, 1),
                       ms_per_step_no_tune=round(1e3 * elapsed_no_tune / args.steps, 4),
                       ms_per_step_eager=round(ms_eager, 4))
        res["gemm_selection"] = ("library default (no tuning pass)" if args.no_tune else
                                 "TunableOp pass in the warm-up" if not args.full else
                                 "TunableOp pass in the warm-up (round 5: the step holds no vendor GEMM any more, so there is nothing to "
                                 "tune — the two legs run the same kernels); ms_per_step_no_tune = the leg without it; ms_per_step_eager = "
                                 "the same step launched op by op without the hipGraph (what an eager training loop gets)")
        if world == 1 and args.full and not args.no_cpu_baseline:
            # the port scales badly past a few dozen threads (tiny per-op work): sweep 8 / 32 / all PHYSICAL cores (BASELINE.md
            # §3), report the fastest leg; the physical core count of the host is stated either way
            pc = physical_cores()
            legs = [cpu_baseline(w, B, grapher, label, x, e, cot_x, cot_e, budget_s=8.0, threads=t)
                    for t in sorted({min(8, pc), min(32, pc), pc})]
            res["cpu_baseline"] = max(legs, key=lambda l: l["value"])
            res["cpu_baseline"]["host_physical_cores"] = pc
            res["cpu_baseline"]["host_logical_cpus"] = os.cpu_count()
            res["cpu_baseline_sweep"] = {str(l["cores"]): l["value"] for l in legs}
            res["speedup_vs_cpu"] = round(value / res["cpu_baseline"]["value"], 1)
        print(json.dumps(res), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
