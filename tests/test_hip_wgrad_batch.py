"""Batched weight gradients (round 5): gkg_linear_wgrad_x6_batch through the C ABI against fp64, and the deferred queue of
gkgnet_amd.fused (weight gradients of a backward pass issued as one launch at its end) against the per-layer launches.
Reference: the weight gradients of torch_vertex.py:290-306 (fc1 / fc2), :334-360 (FFNLabel), torch_nn.py:57-69 (BasicConv)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _problems(shapes, gen):
    from gkgnet_amd import _lib
    ts, ps = [], []
    for R, cin, cout, nb in shapes:
        dy = torch.randn(nb, R, cout, device="cuda", generator=gen)
        x = torch.randn(nb, R, cin, device="cuda", generator=gen) * 2
        dw = torch.zeros(nb, cout, cin, device="cuda")
        ts.append((dy, x, dw))
        ps.append(_lib.WgradProblem(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), R * cout, R * cin, cout, cin, R, cin, cout, nb))
    return ts, ps


def _check(ts):
    for dy, x, dw in ts:
        ref = torch.bmm(dy.double().transpose(1, 2), x.double())
        mag = torch.bmm(dy.double().abs().transpose(1, 2), x.double().abs()) + 1e-30
        e = float(((dw.double() - ref).abs() / mag).max())
        f = float(((torch.bmm(dy.transpose(1, 2), x).double() - ref).abs() / mag).max())
        assert e <= max(f, 1.2e-7) and e < 2e-7, (tuple(dy.shape), tuple(x.shape), e, f)


# the eight weight gradients of the cfg2 step (Grapher rows 10 368, label rows 2 560)
CFG2 = [(2560, 1280, 320, 1), (2560, 320, 1280, 1), (2560, 640, 320, 1), (2560, 160, 160, 4), (2560, 320, 320, 1),
        (10368, 640, 320, 1), (10368, 160, 160, 4), (10368, 320, 320, 1)]
# ragged rows (register-load remainder + its own launch), fewer than 12 / 24 / 48 units (1 / 2 / 4 slabs shared by XCDs), one
# unit, unaligned widths (falls out of the batch), three slabs' worth that does not divide 8
ODD = [(777, 36, 40, 1), (1280, 64, 64, 1), (128, 32, 64, 1), (3000, 1, 3, 1), (640, 256, 100, 2), (4100, 400, 100, 1),
       (5120, 80, 80, 1), (19, 16, 8, 1), (2048 + 128 * 9, 200, 72, 1), (129, 64, 8, 2)]


# GKGNet-576's stage widths (80 / 160 / 400, grouped 40): widths that pad to the 64 x 128 and 64 x 64 tile forms in one launch
STAGES = [(6400, 80, 80, 1), (6400, 160, 80, 1), (6400, 80, 320, 1), (6400, 320, 80, 1), (5120, 40, 40, 4), (3200, 160, 160, 1),
          (3200, 160, 640, 1), (1296, 400, 400, 1), (1296, 1600, 400, 1), (2560, 320, 320, 1)]


@pytest.mark.parametrize("shapes", [CFG2, ODD, CFG2 + ODD + CFG2[:3], STAGES], ids=["cfg2", "odd", "two_launches", "stage_widths"])
def test_batch_matches_fp64(shapes):
    from gkgnet_amd import _lib
    lib = _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(len(shapes))
    ts, ps = _problems(shapes, gen)
    arr = (_lib.WgradProblem * len(ps))(*ps)
    _lib.check(lib.gkg_linear_wgrad_x6_batch(arr, len(ps), 0, None), "gkg_linear_wgrad_x6_batch")
    torch.cuda.synchronize()
    _check(ts)


def test_batch_rejects_bad_arguments():
    from gkgnet_amd import _lib
    lib = _lib.load()
    assert lib.gkg_linear_wgrad_x6_batch(None, 1, 0, None) != 0
    p = (_lib.WgradProblem * 1)(_lib.WgradProblem(None, None, None, 0, 0, 4, 4, 128, 4, 4, 1))
    assert lib.gkg_linear_wgrad_x6_batch(p, 1, 0, None) != 0
    assert b"null" in lib.gkg_last_error_string()


def _block_grads(batch: bool, graph: bool, monkeypatch):
    """Parameter gradients of one Grapher -> GrapherLabel fwd+bwd step with a GradBucket."""
    from gkgnet_amd import fused, parallel
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    from gkgnet_amd.wgrad_queue import QUEUE
    monkeypatch.setattr(fused, "WGRAD_BATCH", batch)
    torch.manual_seed(3)
    C, H, L, B = 64, 16, 24, 8                      # T = 2048 rows (whole units), label rows 192 (ragged: own launches)
    g = Grapher(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=True, use_multi_group=True,
                num_group=2).cuda().train()
    gl = GrapherLabel(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=False, num_nodes=L,
                      use_multi_group=True, num_group=2).cuda().train()
    params = list(g.parameters()) + list(gl.parameters())
    bucket = parallel.GradBucket(params)
    x = torch.randn(B, C, H, H, device="cuda").requires_grad_(True)
    e = torch.randn(B, L, C, device="cuda").requires_grad_(True)
    cx, ce = torch.randn(B, C, H, H, device="cuda"), torch.randn(B, L, C, device="cuda")

    def step():
        bucket.release(prezero=True)
        x.grad = None
        e.grad = None
        out = g(x)
        e2, _ = gl(e, out)
        torch.autograd.backward([out, e2], [cx, ce])
        bucket.pack()

    step()
    torch.cuda.synchronize()
    if graph:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step()
        bucket.flat.fill_(float("nan"))
        gr.replay()
        gr.replay()
    torch.cuda.synchronize()
    assert not QUEUE.items and not QUEUE.keep
    return bucket.flat.clone(), x.grad.clone(), e.grad.clone()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipgraph"])
def test_deferred_queue_gives_the_per_layer_gradients(graph, monkeypatch):
    a = _block_grads(True, graph, monkeypatch)
    b = _block_grads(False, False, monkeypatch)
    for u, v in zip(a, b):
        assert torch.isfinite(u).all()
        scale = float(v.abs().max())
        assert float((u - v).abs().max()) <= 2e-5 * scale, float((u - v).abs().max()) / scale


def test_without_a_bucket_nothing_is_queued(monkeypatch):
    from gkgnet_amd import fused
    from gkgnet_amd.grapher import Grapher
    from gkgnet_amd.wgrad_queue import QUEUE
    monkeypatch.setattr(fused, "WGRAD_BATCH", True)
    torch.manual_seed(0)
    g = Grapher(32, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=256, relative_pos=True, use_multi_group=True,
                num_group=2).cuda().train()
    x = torch.randn(8, 32, 16, 16, device="cuda").requires_grad_(True)
    g(x).sum().backward()
    assert not QUEUE.items and not QUEUE.keep
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in g.parameters() if p.requires_grad and p.dim() > 1)


def test_backward_on_a_side_stream_launches_the_batch_there(monkeypatch):
    """Forward and backward under a non-default stream, the engine callback fires in the calling thread: the batch must go to
    the stream its operands were produced on (gradients complete and correct after synchronising THAT stream only)."""
    from gkgnet_amd import fused, parallel
    from gkgnet_amd.grapher import Grapher
    monkeypatch.setattr(fused, "WGRAD_BATCH", True)
    torch.manual_seed(5)
    g = Grapher(64, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=256, relative_pos=True, use_multi_group=True,
                num_group=2).cuda().train()
    x = torch.randn(8, 64, 16, 16, device="cuda").requires_grad_(True)
    cot = torch.randn(8, 64, 16, 16, device="cuda")
    params = list(g.parameters())
    # reference gradients: per-layer launches on the default stream
    monkeypatch.setattr(fused, "WGRAD_BATCH", False)
    g(x).backward(cot)
    torch.cuda.synchronize()
    want = {n: p.grad.clone() for n, p in g.named_parameters() if p.grad is not None}
    g.zero_grad(set_to_none=True)
    x.grad = None
    monkeypatch.setattr(fused, "WGRAD_BATCH", True)
    bucket = parallel.GradBucket(params)
    bucket.release(prezero=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = g(x)
        out.backward(cot)
    s.synchronize()                                     # only the side stream
    got = {n: p.grad for n, p in g.named_parameters() if p.grad is not None}
    for n, v in want.items():
        assert float((got[n] - v).abs().max()) <= 2e-5 * float(v.abs().max()) + 5e-5, n
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- queue overflow
# A cap reached while a block's problems enter the queue: the block driver hands fused._wgrad_defer_block its 3 (Grapher) or
# 5 (GrapherLabel) problems with ONE keep-alive tuple (the arenas every one of them reads).  A launch forced by WgradQueue.MAX /
# MAX_BYTES clears q.keep, so it must come before the first or after the last problem of a block, never in between.
def _three_blocks(monkeypatch, max_items=None, max_bytes=None, batch=True, record=None):
    """Two Graphers and a GrapherLabel through the block driver with bucket slots; one fwd + bwd step.  Backward order: the label
    block (5 problems), then the two Graphers (3 + 3).  T = 32 * 144 = 4608 rows (36 units of 128 rows: two slabs per weight
    gradient, so their fp32 atomic accumulation into the zeroed slot is order-independent and dW reproducible bit for bit), label
    rows 32 * 16 = 512.  -> (flat gradients, dx, de)."""
    from gkgnet_amd import block, fused, parallel
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    from gkgnet_amd.wgrad_queue import QUEUE, WgradQueue
    monkeypatch.setattr(block, "ENABLED", True)
    monkeypatch.setattr(fused, "WGRAD_BATCH", batch)
    if max_items is not None:
        monkeypatch.setattr(WgradQueue, "MAX", max_items)
    if max_bytes is not None:
        monkeypatch.setattr(WgradQueue, "MAX_BYTES", max_bytes)
    block._PLANS.clear()
    torch.manual_seed(13)
    C, H, L, B, G = 64, 12, 16, 32, 2
    mk = lambda: Grapher(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=True, use_multi_group=True,      # noqa: E731
                         num_group=G).cuda().train()
    g1, g2 = mk(), mk()
    gl = GrapherLabel(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, relative_pos=False, num_nodes=L,
                      use_multi_group=True, num_group=G).cuda().train()
    params = list(g1.parameters()) + list(g2.parameters()) + list(gl.parameters())
    bucket = parallel.GradBucket(params)
    gen = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn(B, C, H, H, device="cuda", generator=gen).requires_grad_(True)
    e = torch.randn(B, L, C, device="cuda", generator=gen).requires_grad_(True)
    cx, ce = torch.randn(B, C, H, H, device="cuda", generator=gen), torch.randn(B, L, C, device="cuda", generator=gen)
    bucket.release(prezero=True)
    if record is not None:
        real_defer, real_launch = fused._wgrad_defer_block, WgradQueue._launch_batch

        def op_bytes(p):
            return 4 * p.nb * p.R * (p.cin + p.cout)                       # the (dY, x) pair of one problem, fp32

        def launch(q, arr, n):
            record["launches"].append((n, q.bytes, sum(op_bytes(arr[i]) for i in range(n))))
            return real_launch(q, arr, n)

        def defer(problems, n, outs, keep, device):
            q = QUEUE
            taken = real_defer(problems, n, outs, keep, device)
            mine = {problems[i].dw for i in range(n)}
            record["blocks"].append(dict(taken=taken, n=n, items=len(q.items), keeps=len(q.keep), bytes=q.bytes,
                                         want_bytes=sum(op_bytes(p) for p in q.items),
                                         held=all(kp is not None and all(any(t is u for u in kp) for t in keep)
                                                  for p, kp in zip(q.items, q.keep) if p.dw in mine)))
            return taken
        monkeypatch.setattr(WgradQueue, "_launch_batch", launch)
        monkeypatch.setattr(fused, "_wgrad_defer_block", defer)
    out = g2(g1(x))
    e2, _ = gl(e, out)
    torch.autograd.backward([out, e2], [cx, ce])
    bucket.pack()
    torch.cuda.synchronize()
    assert not QUEUE.items and not QUEUE.keep and QUEUE.bytes == 0
    return bucket.flat.clone(), x.grad.clone(), e.grad.clone()


def test_a_cap_reached_inside_a_block_keeps_the_blocks_operands_alive(monkeypatch):
    """MAX = 4: the label block's five problems overflow the queue on their own, and the second Grapher's three do not fit behind
    the first one's.  After every block: one keep entry per queued problem, every queued problem of the block holds the block's
    keep tuple, and q.bytes is the real operand byte count of what is queued (it was 0 for blocks: MAX_BYTES never saw them)."""
    rec = {"blocks": [], "launches": []}
    _three_blocks(monkeypatch, max_items=4, record=rec)
    assert [b["n"] for b in rec["blocks"]] == [5, 3, 3] and all(b["taken"] for b in rec["blocks"])      # the driver, with bucket slots
    for b in rec["blocks"]:
        assert b["keeps"] == b["items"], b
        assert b["held"], b
        assert b["bytes"] == b["want_bytes"], b
    assert [b["items"] for b in rec["blocks"]] == [0, 3, 3]                # 5 >= MAX: launched whole; 3; 3 + 3 > MAX: launched, then 3
    assert [n for n, _, _ in rec["launches"]] == [5, 3, 3]                 # never a part of a block
    assert all(have == want and want > 0 for _, have, want in rec["launches"])


@pytest.mark.parametrize("cap", [dict(max_items=4), dict(max_bytes=1 << 20)], ids=["MAX", "MAX_BYTES"])
def test_gradients_under_overflow_are_those_of_the_default_queue(cap, monkeypatch):
    """Every gradient bit for bit as with the default caps: where the queue is cut changes which launch computes a dW, not its
    value.  (The BN column sums of the forward are accumulated with fp64 atomics and a mean on an fp32 rounding tie can differ
    between two runs of the SAME configuration — tests/test_hip_block_driver.py — so a pair that differs is repeated; a real
    difference shows in every pair.)  And to rounding as the per-layer launches (GKG_DISABLE=wgrad_batch), at this file's tolerance."""
    TIE = 2e-5                    # what a BN mean one ulp apart moves any gradient by, at most (the bound this file uses throughout)
    same = False
    for attempt in range(4):
        small = _three_blocks(monkeypatch, **cap)
        monkeypatch.undo()
        default = _three_blocks(monkeypatch)
        monkeypatch.undo()
        # EVERY pair, agreeing bit for bit or not, agrees to rounding: a dW computed from a released arena is wrong by far more than
        # a tie is, and is not repeated away
        for u, v in zip(small, default):
            assert torch.isfinite(u).all()
            scale = float(v.abs().max())
            assert float((u - v).abs().max()) <= TIE * scale, (attempt, float((u - v).abs().max()) / scale)
        same = all(torch.equal(u, v) for u, v in zip(small, default))
        if same:
            break
    assert same
    per_layer = _three_blocks(monkeypatch, batch=False)
    for u, w in zip(small, per_layer):
        scale = float(w.abs().max())
        assert float((u - w).abs().max()) <= 2e-5 * scale, float((u - w).abs().max()) / scale


def test_a_block_that_exactly_fills_the_queue_leaves_nothing_dangling(monkeypatch):
    """MAX = 6: the label block (5) stays queued, the first Grapher (5 + 3 > 6) sends it out and queues 3, the second one makes
    len(items) + n == MAX: all six go out together and the queue is empty, keep list included."""
    rec = {"blocks": [], "launches": []}
    _three_blocks(monkeypatch, max_items=6, record=rec)
    assert [b["items"] for b in rec["blocks"]] == [5, 3, 0]
    assert [b["keeps"] for b in rec["blocks"]] == [5, 3, 0] and all(b["held"] for b in rec["blocks"])
    assert [b["bytes"] for b in rec["blocks"]] == [b["want_bytes"] for b in rec["blocks"]] and rec["blocks"][2]["bytes"] == 0
    assert [n for n, _, _ in rec["launches"]] == [5, 6]
