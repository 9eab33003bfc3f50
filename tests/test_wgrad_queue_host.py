"""The host-side protocol of the deferred weight-gradient queue (gkgnet_amd/wgrad_queue.py) on the CPU: the real WgradQueue with
the graph-task id, the raw streams, the engine callback, the C call and the event wait scripted by the test.  Problems are real
_lib.WgradProblem structs with made-up pointers (``dw`` doubles as the problem's name), outputs are CPU tensors dressed as bucket
slots.  After every step of every scenario ``check`` asserts the invariants of the class docstring."""
import gc
import weakref

import pytest
import torch

from gkgnet_amd import _lib
from gkgnet_amd.wgrad_queue import WgradQueue


def _op_bytes(p):
    return 4 * p.nb * p.R * (p.cin + p.cout)               # the (dY, x) pair of one problem, fp32


class _Owner:
    pass


class _Arena:
    """A keep-alive object the test can hold by weak reference."""


def _slot(owner=True):
    t = torch.zeros(1)
    t._gkg_slot = True
    if owner:
        t._gkg_owner = _Owner()
    return t


class _Sim(WgradQueue):
    def __init__(self, max_items=None, max_bytes=None):
        super().__init__()
        if max_items is not None:
            self.MAX = max_items
        if max_bytes is not None:
            self.MAX_BYTES = max_bytes
        self.now_task, self.raw, self.caller, self.dev = 1, 10, None, "gpu0"
        self.callbacks, self.waits, self.fail = 0, 0, None
        self.launches = []               # one dict per C call, failed ones included
        self.pushes, self.where, self.watch, self.names = [], {}, [], 0

    # ---- the seams
    def task_id(self):
        return self.now_task

    def _raw_stream(self, device=None):
        if device is None:
            return self.raw
        assert device == self.device
        return self.raw if self.caller is None else self.caller

    def _on_backward_end(self):
        self.callbacks += 1

    def _launch_batch(self, arr, n):
        assert n == len(arr) > 0 and not self.items
        self.launches.append(dict(n=n, dws=[arr[i].dw for i in range(n)], stream=self.stream, device=self.device, units=self.units,
                                  bytes=self.bytes, want_bytes=sum(_op_bytes(arr[i]) for i in range(n)),
                                  keep=[id(k) for k in self.keep], alive=[w() is not None for w in self.watch]))
        if self.fail is not None:
            raise self.fail

    def _order_caller_behind(self):
        self.waits += 1

    # ---- what fused does with the queue
    def put(self, n=1, keep=None, R=256, cin=8, cout=4, nb=1, units=0):
        """One autograd node: open for the running pass on the current stream, then ONE push of n problems."""
        q = self.open(self.task_id(), self.dev, units)
        assert q is self
        ps = [_lib.WgradProblem(0x1000, 0x2000, 0x100000 + 16 * (self.names + i), 0, 0, cout, cin, R, cin, cout, nb, 0)
              for i in range(n)]
        self.names += n
        outs = [_slot() for _ in ps]
        self.pushes.append({p.dw for p in ps})
        for p in ps:
            self.where[p.dw] = (self.raw, self.dev)
        try:
            self.push(ps, outs, (ps, outs) if keep is None else keep)
        finally:
            self.check()
        return ps, outs

    def check(self):
        assert len(self.items) == len(self.keep)
        assert self.bytes == sum(_op_bytes(p) for p in self.items)
        assert len(self.items) < self.MAX and self.bytes <= self.MAX_BYTES
        seen = set()
        for rec in self.launches:
            dws = set(rec["dws"])
            assert len(dws) == rec["n"] and not dws & seen, "a problem launched twice"
            seen |= dws
            assert all(p <= dws or not p & dws for p in self.pushes), "a launch holds part of a push"
            assert {self.where[d] for d in dws} == {(rec["stream"], rec["device"])}, "launched elsewhere than queued"
            assert rec["bytes"] == rec["want_bytes"] > 0 and len(rec["keep"]) == rec["n"]
        assert not seen & {p.dw for p in self.items}

    def end(self):
        """The engine callback at the end of the pass."""
        try:
            self.flush()
        finally:
            self.check()

    def sizes(self):
        return [rec["n"] for rec in self.launches]


def test_singles_up_to_max_go_out_in_one_launch():
    q = _Sim()
    for i in range(q.MAX):
        assert q.sizes() == [] and len(q.items) == i
        q.put()
    assert q.sizes() == [WgradQueue.MAX] and not q.items and not q.keep and q.bytes == 0
    q.end()
    assert q.sizes() == [WgradQueue.MAX] and q.callbacks == 1


def test_max_bytes_launches_with_the_push_that_crosses_it():
    one = 4 * 2 * 256 * (8 + 4)                            # nb = 2 problems of 256 rows, 8 -> 4 columns
    q = _Sim(max_bytes=3 * one)
    for i in range(3):
        q.put(nb=2)
        assert q.sizes() == [] and q.bytes == (i + 1) * one
    q.put(nb=2)
    assert q.sizes() == [4] and q.launches[0]["bytes"] == 4 * one == q.launches[0]["want_bytes"]
    assert not q.items and q.bytes == 0
    q.put(3, nb=2, R=512)                                  # one push, 6 * one on its own: goes out whole, after its last problem
    assert q.sizes() == [4, 3] and q.launches[1]["bytes"] == 6 * one


@pytest.mark.parametrize("max_items, launches, left", [(4, [5, 3, 3], [0, 3, 3]), (6, [5, 6], [5, 3, 0])])
def test_blocks_are_never_split(max_items, launches, left):
    """The two cases tests/test_hip_wgrad_batch.py pins on the device: a label block (5 problems), then two Graphers (3 + 3)."""
    q = _Sim(max_items=max_items)
    queued = []
    for n in (5, 3, 3):
        arena = _Arena()
        q.put(n, keep=arena)
        queued.append(len(q.items))
        assert all(k is arena for k in q.keep[len(q.keep) - min(n, len(q.keep)):])
    q.end()
    assert queued == left and q.sizes() == launches
    assert not q.items and not q.keep and q.bytes == 0


def test_keep_alives_live_until_their_launch_and_no_longer():
    q = _Sim()
    single, block = _Arena(), _Arena()
    refs = [weakref.ref(single), weakref.ref(block)]
    q.watch = refs
    q.put(1, keep=single)
    q.put(3, keep=block)
    assert q.keep[0] is single and all(k is block for k in q.keep[1:]) and len(q.keep) == 4     # every entry of the block
    del single, block
    gc.collect()
    assert all(r() is not None for r in refs)              # the queue is what holds them now
    q.end()
    assert q.sizes() == [4] and q.launches[0]["alive"] == [True, True]
    gc.collect()
    assert all(r() is None for r in refs)


def test_a_new_task_launches_what_the_old_one_left_where_it_was_queued():
    q = _Sim()
    q.put()
    q.put(3)
    assert q.callbacks == 1                                # once per task, not once per push
    q.now_task, q.raw, q.dev = 2, 11, "gpu1"               # the first pass never reached its callback
    q.put(2, units=7)
    assert q.sizes() == [4] and (q.launches[0]["stream"], q.launches[0]["device"]) == (10, "gpu0")
    assert q.callbacks == 2 and len(q.items) == 2 and q.task == 2
    q.put(units=7)
    assert q.callbacks == 2
    q.end()
    assert q.sizes() == [4, 3] and (q.launches[1]["stream"], q.launches[1]["device"], q.launches[1]["units"]) == (11, "gpu1", 7)
    assert q.task == -1


@pytest.mark.parametrize("what", ["stream", "device"])
def test_the_same_task_elsewhere_sends_the_queue_out_first(what):
    q = _Sim()
    q.put(2)
    if what == "stream":
        q.raw = 11
    else:
        q.dev = "gpu1"
    new, _ = q.put(1)
    assert q.sizes() == [2] and (q.launches[0]["stream"], q.launches[0]["device"]) == (10, "gpu0")
    assert [p.dw for p in q.items] == [new[0].dw] and len(q.keep) == 1 and q.callbacks == 1
    q.end()
    assert q.sizes() == [2, 1] and (q.launches[1]["stream"], q.launches[1]["device"]) == (q.raw, q.dev)


def test_flush_on_an_empty_queue_only_resets():
    q = _Sim()
    q.end()
    assert q.launches == [] and q.waits == 0 and q.task == -1
    q.put()
    q.end()
    q.end()                                                # GradBucket's flush after the engine's
    assert q.sizes() == [1] and q.task == -1 and not q.keep and q.bytes == 0
    q.put()
    assert q.callbacks == 2                                # the same task id after a flush is a pass of its own


def test_flush_orders_a_caller_on_another_stream_behind_the_batch():
    q = _Sim()
    q.put(2)
    q.end()                                                # the caller's stream is the queue's
    assert q.sizes() == [2] and q.waits == 0
    q.now_task = 2
    q.put(2)
    q.caller = 12
    q.end()
    assert q.sizes() == [2, 2] and q.waits == 1
    q.end()                                                # nothing was launched: nothing to wait for
    assert q.waits == 1


@pytest.mark.parametrize("via", ["flush", "push", "open"])
def test_a_launch_that_raises_releases_everything(via):
    q = _Sim(max_items=3)
    arena = _Arena()
    ref = weakref.ref(arena)
    q.put(2, keep=arena)
    del arena
    q.fail = RuntimeError("launch failed")
    with pytest.raises(RuntimeError, match="launch failed"):
        if via == "flush":
            q.end()
        elif via == "push":
            q.put(1)                                       # reaches MAX
        else:
            q.now_task = 2
            q.put(1)                                       # the new pass sends the old one's problems out first
    failed = 3 if via == "push" else 2
    assert q.sizes() == [failed] and not q.items and not q.keep and q.bytes == 0
    gc.collect()
    assert ref() is None
    q.fail = None
    q.end()
    assert q.sizes() == [failed]                           # not launched a second time
    q.now_task = 3
    q.put(2)
    q.end()
    assert q.sizes() == [failed, 2] and q.task == -1 and q.waits == 0


def test_push_marks_the_owner_and_touches_nothing_else():
    q = _Sim()
    _, outs = q.put(3)
    assert all(o._gkg_owner._gkg_deferred is True for o in outs)
    bare = _slot(owner=False)
    p = _lib.WgradProblem(0x1000, 0x2000, 0x3000, 0, 0, 4, 8, 128, 8, 4, 1, 0)
    q.push([p], [bare], None)
    assert not hasattr(bare, "_gkg_owner") and not hasattr(bare, "_gkg_deferred") and len(q.items) == len(q.keep) == 4
    assert q.bytes == 3 * _op_bytes(q.items[0]) + 4 * 128 * 12
