"""Per-device fp64 column-sum scratch of the two-launch BN passes (gkg_bn_apply_train / gkg_bn_bwd_atomic): the host-side
protocol of the two alternating buffers — which one is clean, who clears the other, what a hipGraph capture, a failed launch
and a statistics hand-off between two autograd nodes do to that."""
from __future__ import annotations

import torch

from . import _lib
from .ops import _stream


class _BnLink:
    """A BN layer as its passes read it (bn_passes.py): the saved tensors, the sizes, ``sync`` = (group, count) of exchanged
    statistics and, for a layer on its running statistics (``mean`` None), the module and the conv bias in front of it.  A
    train-mode layer with rank-local statistics may hang it on the tensor it returns: the kernel that writes that tensor's
    gradient also takes the layer's BN backward statistics and leaves them here (_BnScratch.hand_off / take)."""
    __slots__ = ("Y", "a", "c", "mean", "invstd", "act", "nb", "co", "R", "sync", "bn", "bias", "ready", "__weakref__")

    def __init__(self, Y, a, c, mean, invstd, act, nb, co, R, sync=None, bn=None, bias=None):
        self.Y, self.a, self.c, self.mean, self.invstd, self.act, self.nb, self.co, self.R = Y, a, c, mean, invstd, act, nb, co, R
        self.sync, self.bn, self.bias = sync, bn, bias
        self.ready = None             # (the gradient tensor the sums belong to, its version, cur, other, zero)

    def holds_sums(self) -> bool:
        return self.ready is not None


class _BnScratch:
    """Two fp64 column-sum buffers per device for gkg_bn_apply_train / gkg_bn_bwd_atomic, used alternately by forward and
    backward passes alike: a call accumulates into the clean one and its apply pass clears what the previous call left in the
    other (stream-ordered, single stream: like _stats_scratch).  ``dirty[i]``: doubles of buffer i that hold sums.

    Who calls what (nothing outside this module touches the state): a BN pass asks ``fits(n)`` and issues its launches inside
    ``with scoped(lib, n) as (cur, other, zero)``; the block driver calls acquire() once per layer inside ``with one_call()``; a
    kernel that takes ANOTHER layer's statistics while it writes that layer's gradient does so in a scoped pass and leaves them
    with ``hand_off``, the layer's backward asks with ``take`` and runs its apply pass inside ``with scratch``; the weight-plane
    refresh uses ``existing`` and ``fold_reset``.  A body that raises leaves sums behind that the bookkeeping calls clean: each
    of the three with-blocks then marks the pair, and the next acquire clears both buffers.

    hipGraph captures make the host-side bookkeeping blind (a replay runs its calls without this object seeing them), so:
    the FIRST call of every capture clears both buffers inside the capture (one memset pair per replay: the replayed
    sequence is self-contained), and once any capture exists every EAGER call clears both buffers first (correct after any
    interleaving of replays and eager calls; only mixed capture / eager use pays for it).

    Streams: the pair is shared by every stream of the device.  Eager calls from a stream other than the previous
    eager caller's first wait for that stream (``wait_stream``: everything the previous user enqueued, its apply pass
    included, completes before this call's atomics start), so blocks driven from two streams by ONE host thread — a
    side-stream evaluation during training — serialise on the pair instead of mixing their sums.  Concurrent host THREADS
    are not supported (like the rest of the fused path's per-device scratch).

    What the protocol asks of the device sits in _capture_id, _raw_stream, _current_stream and _reset's fill of ``store``:
    tests/test_bn_scratch_host.py drives the state machine with a CPU ``store`` and scripted answers."""
    DOUBLES = 2 * 4096 * 4
    _inst = {}

    def __init__(self, device):
        self.store = torch.zeros((2, self.DOUBLES), dtype=torch.float64, device=device)
        self.bufs = [self.store[0], self.store[1]]
        self.cur = 0
        self.dirty = [0, 0]
        self.capture_id = 0
        self.captured = False
        self.poisoned = False           # a launch between an acquire and its apply pass failed: the buffers' contents are unknown
        self.last_stream = None
        self.last_raw = None
        self.hold = 0                   # one_call(): 1 = the next acquire may reset, 2 = later acquires of the same call may not
        self.pending = None             # a _BnLink whose consumer has accumulated into a buffer while the clear of the other one
                                        # waits for the producer's apply pass (hand_off)
        self._scoped = None             # what scoped() acquired, for __enter__

    @classmethod
    def of(cls, device):
        key = (device.type, device.index)
        inst = cls._inst.get(key)
        if inst is None:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.GkgError("BN scratch first used inside a hipGraph capture; run one eager warm-up step first")
            inst = cls._inst[key] = cls(device)
        return inst

    @classmethod
    def existing(cls, device):
        """The device's instance, or None when no BN pass has used the pair yet (never creates one: safe inside a capture)."""
        return cls._inst.get((device.type, device.index))

    @classmethod
    def fits(cls, n) -> bool:
        return n <= cls.DOUBLES

    def _capture_id(self, lib) -> int:
        return lib.gkg_stream_capture_id(_stream()) if torch.cuda.is_current_stream_capturing() else 0

    def _raw_stream(self):
        return _stream()

    def _current_stream(self):
        return torch.cuda.current_stream(self.store.device)

    def acquire(self, lib, n):
        """-> (buffer to accumulate into: clean, buffer to clear, doubles to clear); the caller's kernels do the clearing."""
        cap = self._capture_id(lib)
        if cap:
            self.captured = True
            if cap != self.capture_id:
                self.capture_id = cap
                self._reset()
        else:
            raw = self._raw_stream()
            if self.last_raw != raw:                    # (Stream objects only when the caller's stream actually changed)
                here = self._current_stream()
                if self.last_stream is not None and self.last_stream != here:
                    here.wait_stream(self.last_stream)
                self.last_stream = here
                self.last_raw = raw
            if (self.captured or self.poisoned) and self.hold != 2:
                self._reset()
        if self.pending is not None:
            # an acquire between a consumer's hand_off and its producer's apply pass (another ready BN backward node was
            # scheduled in between, or the producer's backward never ran: autograd.grad stopping at the activation): the
            # deferred clear has not happened and the bookkeeping calls that buffer clean -> start clean, and the
            # producer falls back to its own statistics pass
            self._reset()
        cur, other = self.bufs[self.cur], self.bufs[self.cur ^ 1]
        zero = self.dirty[self.cur ^ 1]
        self.dirty[self.cur], self.dirty[self.cur ^ 1] = n, 0
        self.cur ^= 1
        if self.hold == 1:
            self.hold = 2
        return cur, other, zero

    def scoped(self, lib, n):
        """``with scratch.scoped(lib, n) as (cur, other, zero)``: acquire() for one pass whose launches the body issues."""
        self._scoped = self.acquire(lib, n)
        return self

    def __enter__(self):
        return self._scoped

    def __exit__(self, et, ev, tb):
        self.hold = 0
        if et is not None:
            self.poisoned = True
        return False

    def one_call(self):
        """Several acquire() calls whose launches are all issued afterwards, together (the block driver fills every layer's
        descriptor first): the clear that an eager call owes after a capture or a failed launch is enqueued by the FIRST
        acquire only — a later one would clear, ahead of the block's launches, a buffer the bookkeeping then hands to a layer
        while an earlier layer's sums are still in it.  (The with-blocks do not nest.)"""
        self.hold = 1
        return self

    def hand_off(self, link, tensor, cur, other, zero):
        """``cur`` holds ``link``'s BN backward statistics of the gradient ``tensor``; the clear of ``other`` waits for that layer's
        apply pass.  The tensor ITSELF and its version are kept: holding it keeps autograd from accumulating another
        consumer's gradient into it in place (use_count > 1 -> a fresh sum is allocated), and a changed version or another object
        means the sums do not describe the gradient the layer receives."""
        link.ready = (tensor, tensor._version, cur, other, zero)
        self.pending = link

    def take(self, link, g, same_layout=True):
        """-> (cur, other, zero) for the apply pass of ``link``'s layer, whose gradient ``g`` arrived (``same_layout``: with the
        strides the statistics were taken with), or None: run the statistics pass.  Sums of another gradient (autograd added a
        second contribution) leave the buffer bookkeeping off by one acquire -> start clean."""
        if link.ready is None:
            return None
        tensor, version, cur, other, zero = link.ready
        link.ready = None
        if self.pending is link:
            self.pending = None
        if g is tensor and g._version == version and same_layout:
            return cur, other, zero
        self.poisoned = True
        return None

    def fold_reset(self, cap):
        """The first use of the pair inside hipGraph capture ``cap`` would clear both buffers with a launch of its own: when the
        weight-plane refresh (the first launch of a captured step) runs first, it clears them in ITS launch — returns the storage
        to clear, or None when this capture has already been seen."""
        if not cap or cap == self.capture_id:
            return None
        self.captured = True
        self.capture_id = cap
        self.dirty = [0, 0]
        self.poisoned = False
        self._drop_pending()
        return self.store

    def _reset(self):
        self.store.fill_(0.0)            # ONE elementwise launch (a captured memset node measured far slower than a kernel node)
        self.dirty = [0, 0]
        self.poisoned = False
        self._drop_pending()

    def _drop_pending(self):
        if self.pending is not None:
            self.pending.ready = None
            self.pending = None
