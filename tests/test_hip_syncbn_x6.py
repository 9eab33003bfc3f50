"""SyncBatchNorm layers on the split-bf16 projection path: two gloo ranks sharing GPU 0 (as tests/test_hip_syncbn.py), the batch
split 3 + 5 so that the exchanged row count matters.  Under GKG_GEMM_MATH=x6 a SyncBN layer runs the x6 forward / input-gradient /
weight-gradient GEMMs (fused._mm_t, the vendor-library projection, is never called), its statistics travel as ONE fp64 all-reduce
per direction — a slice of the BN scratch pair, sums and row count together — and everything equals the single-process full-batch
plain-BN run to the tolerances of tests/test_hip_syncbn.py.  With DropPath active (the scale of the incoming gradient is applied
inside the two BN-backward launches) it still does; GKG_GEMM_MATH=vendor keeps the fp32 two-stage exchange.

One spawn runs the three configurations; each test reads its verdict."""
import datetime
import os
import tempfile
import traceback

import pytest
import torch

pytestmark = pytest.mark.gpu

SPLIT = (3, 5)
MODES = ("x6", "x6_droppath", "vendor")
DROP_SEED = 26000          # the first two Bernoulli(0.9) masks are [1 1 0 | 0 1 1 1 1]: an image dropped, images kept on either rank


def _build(norm_type, drop_path):
    from gkgnet_amd import layers
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    layers.norm_cfg["type"] = norm_type
    torch.manual_seed(0)
    B, C, H, G, k, L = 8, 64, 10, 4, 9, 12
    g = Grapher(C, k, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, drop_path=drop_path, relative_pos=True,
                use_multi_group=True, num_group=G).cuda().train()
    gl = GrapherLabel(C, k, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, drop_path=drop_path, num_nodes=L,
                      use_multi_group=True, num_group=G).cuda().train()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, H, H, generator=gen).cuda()
    e = torch.randn(B, L, C, generator=gen).cuda()
    cx = torch.randn(B, C, H, H, generator=gen).cuda()
    ce = torch.randn(B, L, C, generator=gen).cuda()
    return g, gl, x, e, cx, ce


def _run(g, gl, x, e, cx, ce):
    xg, eg = x.clone().requires_grad_(True), e.clone().requires_grad_(True)
    out = g(xg)
    e2, _ = gl(eg, out)
    torch.autograd.backward([out, e2], [cx, ce])
    grads = {n: p.grad.clone() for mod, tag in ((g, "g."), (gl, "l.")) for n, p in
             ((tag + n_, p_) for n_, p_ in mod.named_parameters()) if p.grad is not None}
    bufs = {tag + n_: b.clone() for mod, tag in ((g, "g."), (gl, "l.")) for n_, b in mod.named_buffers()
            if "running" in n_ or "num_batches" in n_}
    return out.detach(), e2.detach(), xg.grad, eg.grad, grads, bufs


class _FixedDropPath:
    """DropPath.sample_scale with the draws of the WHOLE batch fixed by a seed (one generator per call of a step) and this rank's
    images cut out of them: the full-batch reference and the two ranks scale the same images."""

    def __init__(self, layers, full_batch):
        self.layers, self.B, self.sl, self.calls = layers, full_batch, slice(0, full_batch), 0

    def __enter__(self):
        me, self.real = self, self.layers.DropPath.sample_scale

        def sample_scale(mod, batch, device, dtype=torch.float32):
            if not mod.active():
                return None
            keep = 1.0 - mod.drop_prob
            gen = torch.Generator().manual_seed(DROP_SEED + me.calls)
            me.calls += 1
            s = (torch.empty(me.B).bernoulli_(keep, generator=gen) / keep)[me.sl]
            assert s.numel() == batch
            return s.to(device=device, dtype=dtype)
        self.layers.DropPath.sample_scale = sample_scale
        return self

    def step(self, sl):
        self.sl, self.calls = sl, 0

    def __exit__(self, *exc):
        self.layers.DropPath.sample_scale = self.real


class _VendorGemms:
    """Counts the library GEMMs issued through torch.mm / bmm / addmm (what every projection, input gradient and weight gradient
    off the x6 kernels ends in)."""
    NAMES = ("mm", "bmm", "addmm")

    def __enter__(self):
        self.n, self.real = 0, {n: getattr(torch, n) for n in self.NAMES}
        for name, fn in self.real.items():
            setattr(torch, name, self._counting(fn))
        return self

    def _counting(self, fn):
        def w(*a, **k):
            self.n += 1
            return fn(*a, **k)
        return w

    def __exit__(self, *exc):
        for name, fn in self.real.items():
            setattr(torch, name, fn)


def _one_mode(mode, rank, dist, fused, layers, drop):
    dp = 0.1 if mode == "x6_droppath" else 0.0
    drop.step(slice(0, 8))
    with _VendorGemms() as vend_ref:
        ref = _run(*_build("BN", dp))              # single process, full batch, local statistics, the same fused kernels
    ref_draws = drop.calls
    g, gl, x, e, cx, ce = _build("SyncBN", dp)
    assert isinstance(g.fc1[1], torch.nn.SyncBatchNorm) and fused._sync_group(g.fc1[1]) is not None
    sl = slice(0, SPLIT[0]) if rank == 0 else slice(SPLIT[0], SPLIT[0] + SPLIT[1])
    drop.step(sl)
    n_bn = sum(isinstance(m, torch.nn.SyncBatchNorm) for mod in (g, gl) for m in mod.modules())
    store = fused._BnScratch.of(x.device).store.untyped_storage().data_ptr()
    mm, reduced, fused_calls = [], [], []
    real_mm, real_ar, real_gf = fused._mm_t, dist.all_reduce, fused.grapher_forward
    fused._mm_t = lambda *a, **k: (mm.append(1), real_mm(*a, **k))[1]
    fused.grapher_forward = lambda *a, **k: (fused_calls.append(1), real_gf(*a, **k))[1]
    dist.all_reduce = lambda t, *a, **k: (reduced.append((t.dtype, t.untyped_storage().data_ptr())), real_ar(t, *a, **k))[1]
    math = fused.GEMM_MATH
    fused.GEMM_MATH = "vendor" if mode == "vendor" else "x6"
    try:
        with _VendorGemms() as vend:
            got = _run(g, gl, x[sl], e[sl], cx[sl], ce[sl])
    finally:
        fused._mm_t, dist.all_reduce, fused.grapher_forward, fused.GEMM_MATH = real_mm, real_ar, real_gf, math
    # every rank takes every collective below whatever it finds: the findings are gathered and raised at the end
    bad = []

    def check(ok, *what):
        if not ok:
            bad.append(what)
    check(fused_calls, "SyncBatchNorm across ranks was expected to stay on the fused path")
    check(n_bn == 8 and len(reduced) == 2 * n_bn, "two collectives per SyncBN layer and step", n_bn, len(reduced))
    if mode == "vendor":
        check(mm, "GKG_GEMM_MATH=vendor: the projections go to the vendor library")
        check(all(dt == torch.float32 for dt, _ in reduced), "fp32 all-reduces", [dt for dt, _ in reduced])
    else:
        check(not mm, f"{len(mm)} projections of SyncBN layers went to the vendor library")
        check(vend.n <= vend_ref.n, "library GEMMs in the step, forward and backward: SyncBN / plain BN", vend.n, vend_ref.n)
        check(all(dt == torch.float64 for dt, _ in reduced), "fp64 all-reduces", [dt for dt, _ in reduced])
        check(all(ptr == store for _, ptr in reduced), "the exchanged tensors are slices of the BN scratch pair")
    if dp:
        check(drop.calls == ref_draws >= 2, "DropPath draws: SyncBN step / reference step", drop.calls, ref_draws)
    tol = dict(atol=2e-4, rtol=1e-3)
    for name, a_, b_ in zip(("out", "labels", "dx", "de"), got[:4], ref[:4]):
        check(torch.allclose(a_, b_[sl], **tol), name, float((a_ - b_[sl]).abs().max()))
    check(sorted(got[4]) == sorted(ref[4]), "parameters with a gradient", sorted(got[4]), sorted(ref[4]))
    for n_ in sorted(ref[4]):                          # parameter gradients add up over the ranks
        tot = got[4][n_].clone() if n_ in got[4] else torch.zeros_like(ref[4][n_])
        dist.all_reduce(tot)
        check(torch.allclose(tot, ref[4][n_], atol=2e-3, rtol=2e-3), n_, float((tot - ref[4][n_]).abs().max()))
    for n_, b_ in got[5].items():                      # running statistics are the global-batch ones on every rank
        check(torch.allclose(b_.float(), ref[5][n_].float(), atol=1e-5, rtol=1e-4), n_)
    assert not bad, (mode, rank, bad)


def _worker(rank, world, store_path, result_path):
    import torch.distributed as dist
    from gkgnet_amd import fused, layers
    torch.cuda.set_device(0)                            # gloo: the ranks share GPU 0
    dist.init_process_group("gloo", store=dist.FileStore(store_path, world), rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))
    try:
        with _FixedDropPath(layers, 8) as drop:
            for mode in MODES:
                # a finding must not leave the other rank waiting in a collective: _one_mode raises behind its last one, so the
                # ranks stay in step whatever either of them found, and the verdict is written per mode
                try:
                    _one_mode(mode, rank, dist, fused, layers, drop)
                    verdict = "ok"
                except AssertionError:
                    verdict = traceback.format_exc()
                with open(f"{result_path}.{mode}.{rank}", "w") as fh:
                    fh.write(verdict)
    finally:
        layers.norm_cfg["type"] = "BN"
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def verdicts():
    import torch.multiprocessing as mp
    world = 2
    out = {}
    with tempfile.TemporaryDirectory() as d:
        store, res = os.path.join(d, "store"), os.path.join(d, "res")
        mp.spawn(_worker, args=(world, store, res), nprocs=world, join=True)
        for mode in MODES:
            for r in range(world):
                path = f"{res}.{mode}.{r}"
                out[mode, r] = open(path).read() if os.path.exists(path) else "not run"
    return out


@pytest.mark.parametrize("mode", MODES)
def test_syncbn_two_ranks_3_plus_5(verdicts, mode):
    """x6: no vendor projection, 2 n_bn fp64 all-reduces, equal to the full-batch run; x6_droppath: the same with drop_path = 0.1
    in train(); vendor: fused.GEMM_MATH = "vendor" takes the old path (vendor projections, fp32 all-reduces)."""
    for r in range(2):
        assert verdicts[mode, r] == "ok", f"rank {r}: {verdicts[mode, r]}"
