"""The deferred weight-gradient queue: the host-side protocol of the ONE batched dW launch at the end of a backward pass
(gkg_linear_wgrad_x6_batch; under GKG_DETERMINISTIC with GKG_ENABLE=wgrad_det its run-independent form, _batch_det, and the
workspace that form needs) — what is queued, what keeps its operands alive, where and when it is launched."""
from __future__ import annotations

import torch

from . import _lib, parallel
from .ops import _stream


class WgradQueue:
    """Nothing downstream of a backward pass reads a weight gradient, so the projections' dW launches are taken OFF the chain of
    dependent launches: while the backward runs they are only queued (operands kept alive), and ONE launch at the end of the
    backward pass (an autograd engine callback) computes all of them (csrc/gkg_gemm_x6.hip wgrad_x6_batch_kernel).  At the cfg2
    shapes the ten weight gradients were ten launches of 50-400 workgroups on 256 CUs, 12-40 us each (195 of 981 us, six of them
    vendor kernels); together they fill the chip.

    Who calls what (nothing outside this module touches the state): fused decides WHETHER a gradient is deferred (its switches,
    the kernel's eligibility, a bucket slot to write to) and asks ``task_id()``; with a backward pass running it calls
    ``open(task, device, units)`` and makes ONE ``push`` per autograd node — a projection's single problem or all the problems of
    a block.  ``flush`` is the engine callback of the pass and what GradBucket calls before it reads a gradient
    (parallel.flush_pending_grads); ``fused.flush_wgrads`` is its public name.

    Invariants (tests/test_wgrad_queue_host.py checks them after every step, on the CPU):
    * ``len(items) == len(keep)``: keep[i] is what keeps items[i]'s operands alive;
    * ``bytes`` is the operand bytes of what is queued;
    * a push is never cut by a launch: a cap sends the queue out before the first or after the last of its problems (a block's
      problems read ONE set of arenas — a launch in between released them with the rest of the block still queued);
    * a launch goes to the stream and device its items were queued on — the engine callback runs in the thread that called
      backward(), whose current stream need not be the backward nodes'  —, and what another pass, stream or device
      left queued is launched there, not dropped;
    * keep-alives live exactly until their launch has been issued (it is stream-ordered behind the operands' producers and ahead
      of their reuse), also when the launch raises: ``_launch`` is the only place that takes items out or releases anything.

    What the protocol asks of torch and the device sits in task_id, _raw_stream, _on_backward_end, _launch_batch and
    _order_caller_behind: the host test scripts those."""
    MAX = 192
    # Operand bytes the queue may keep alive: deferring holds every layer's (dY, x) pair until the batch runs —
    # GKGNet-576's train step peaked at 30.7 GiB against 24.2 before the batching.  Problems that fill the chip on their own gain
    # nothing from the batch (see fused._wgrad_defer) and are launched at once; what is left is flushed early past this cap.
    MAX_BYTES = 1 << 30

    def __init__(self):
        self.items, self.keep, self.bytes, self.task = [], [], 0, -1
        self.stream, self.device = None, None        # where the queued operands are produced: the batch is launched THERE
        self.units = 0                               # rows per workgroup / 128 of that launch (fused.WGRAD_UNITS)
        self.det = False                             # that launch is gkg_linear_wgrad_x6_batch_det (fused.WGRAD_DET)

    def task_id(self) -> int:
        """Id of the backward pass this thread is executing (-1: none — nobody would flush a queue —, or one that builds a graph:
        create_graph makes autograd clone what a node returns, so a slot filled later would never reach p.grad)."""
        task_id = getattr(torch._C, "_current_graph_task_id", None)
        task = task_id() if task_id is not None else -1
        return -1 if torch.is_grad_enabled() else task

    def _raw_stream(self, device=None):
        """The current stream of the current device (None) or of ``device``, as the integer the C ABI takes."""
        return _stream() if device is None else torch.cuda.current_stream(device).cuda_stream

    def _on_backward_end(self):
        torch.autograd.Variable._execution_engine.queue_callback(self.flush)

    def _launch_batch(self, arr, n):
        lib = _lib.load()
        with torch.cuda.device(self.device):
            if self.det:        # the run-independent form: partial tiles into a workspace, added in slab order (no cleared slots)
                ws = det_workspace(self.device, lib.gkg_linear_wgrad_x6_batch_det_workspace_bytes(arr, n, self.units))
                _lib.check(lib.gkg_linear_wgrad_x6_batch_det(arr, n, self.units, ws.data_ptr(), ws.numel(), self.stream),
                           "gkg_linear_wgrad_x6_batch_det")
            else:
                _lib.check(lib.gkg_linear_wgrad_x6_batch(arr, n, self.units, self.stream), "gkg_linear_wgrad_x6_batch")

    def _order_caller_behind(self):
        ev = torch.cuda.Event()
        with torch.cuda.device(self.device):
            ev.record(torch.cuda.ExternalStream(self.stream, device=self.device) if self.stream
                      else torch.cuda.default_stream(self.device))
        torch.cuda.current_stream(self.device).wait_event(ev)

    def open(self, task, device, units=0, det=False):
        """The queue of backward pass ``task`` on the current stream: registers the flush callback on the pass's first use, sends
        what another pass (a nested / re-entrant backward, or one that raised before its callback), stream or device left queued
        out where it was produced.  ``det``: its launch is the run-independent form (what was queued for the other form — slots
        cleared or not — goes out first)."""
        st = self._raw_stream()
        if self.task != task:
            self._launch()
            self.task = task
            self._on_backward_end()
        elif self.items and (self.stream != st or self.device != device or self.det != bool(det)):
            self._launch()
        self.stream, self.device, self.units, self.det = st, device, units, bool(det)
        return self

    def push(self, problems, outs, keep):
        """The _lib.WgradProblem structs of one autograd node, the tensors they write and the ONE object that keeps their
        operands alive, all of them or (after a launch that raised) none."""
        if self.items and len(self.items) + len(problems) > self.MAX:
            self._launch()
        for p, out in zip(problems, outs):
            self.items.append(p)
            self.keep.append(keep)
            owner = getattr(out, "_gkg_owner", None)
            if owner is not None:
                owner._gkg_deferred = True   # the slot, not p.grad, holds this gradient until the batch has run (GradBucket._resident)
            # the problem's (dY, x) pair, fp32.  (A block's arenas in ``keep`` hold more than the operands, and its problems may
            # share an x: the sum errs on the early side of MAX_BYTES, never the late one.)
            self.bytes += 4 * p.nb * p.R * (p.cin + p.cout)
        if len(self.items) >= self.MAX or self.bytes > self.MAX_BYTES:
            self._launch()

    def flush(self):
        """Launch every queued weight gradient (no-op when the queue is empty) and close the pass."""
        self.task = -1
        queued = bool(self.items)
        self._launch()
        # whatever the caller's stream does next with the gradients (pack, clip, the optimiser) is ordered behind the batch
        if queued and self._raw_stream(self.device) != self.stream:
            self._order_caller_behind()

    def _launch(self):
        """Everything queued as one batched launch on the stream and device it was queued on."""
        items, self.items = self.items, []
        try:
            if items:
                self._launch_batch((_lib.WgradProblem * len(items))(*items), len(items))
        finally:
            self.keep, self.bytes = [], 0


_DET_WS = {}


def det_workspace(device, nbytes) -> torch.Tensor:
    """Workspace of the run-independent weight-gradient entry points (gkg_linear_wgrad_x6_det / _batch_det: the slabs' partial
    tiles, include/gkg_hip.h): ONE grow-only buffer per device — its contents mean nothing between calls, and calls on a stream
    are ordered.  A buffer that has to grow inside a hipGraph capture is not kept (it lives in the capture's pool)."""
    key = (device.type, device.index)
    t = _DET_WS.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        if not torch.cuda.is_current_stream_capturing():
            _DET_WS[key] = t
    return t


QUEUE = WgradQueue()
parallel._FLUSH.append(lambda: QUEUE.flush())       # (looked up when called: a profiler may wrap QUEUE.flush)
