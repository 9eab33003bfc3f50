"""The host-side protocol of the fp64 BN sum-scratch pair (gkgnet_amd/bn_scratch.py) on the CPU: the real _BnScratch with a CPU
``store``, the capture id / raw stream / stream objects scripted by the test, and simulated launches that do to the buffers what
the kernels do.  The invariant of every scenario: a buffer handed out is clean at the moment its launch runs, and at the end
nothing sits in either buffer beyond what ``dirty`` accounts for."""
import pytest
import torch

from gkgnet_amd.bn_scratch import _BnLink, _BnScratch


class _Stream:
    def __init__(self, raw, waits):
        self.raw, self.waits = raw, waits

    def __eq__(self, other):
        return self.raw == other.raw

    def wait_stream(self, other):
        self.waits.append((self.raw, other.raw))


class _Sim(_BnScratch):
    def __init__(self):
        super().__init__(torch.device("cpu"))
        self.cap, self.raw, self.waits, self.resets = 0, 1, [], 0

    def _capture_id(self, lib):
        return self.cap

    def _raw_stream(self):
        return self.raw

    def _current_stream(self):
        return _Stream(self.raw, self.waits)

    def _reset(self):
        self.resets += 1
        super()._reset()

    def accounted(self):
        return all(not self.store[i, self.dirty[i]:].any() for i in (0, 1))


def _stats(bufs, n):
    """The statistics half of a pass: fp64 atomics into the clean buffer."""
    cur = bufs[0]
    assert not cur[:n].any(), "a buffer handed out as clean holds sums"
    cur[:n] += 1.5


def _apply(bufs):
    """The apply half: clears what the previous pass left in the other buffer."""
    _, other, zero = bufs
    other[:zero] = 0.0


def _launch(bufs, n):
    _stats(bufs, n)
    _apply(bufs)


def _pass(s, n):
    with s.scoped(None, n) as bufs:
        _launch(bufs, n)
    return bufs


@pytest.mark.parametrize("sizes", [(16, 16, 16), (16, 16, 16, 16), (8, 128, 32, 64, 8)])
def test_alternation(sizes):
    s = _Sim()
    seen = []
    for n in sizes:
        seen.append(_pass(s, n)[0].data_ptr())
    assert seen[0] != seen[1] and seen[::2] == [seen[0]] * len(seen[::2]) and seen[1::2] == [seen[1]] * len(seen[1::2])
    assert s.resets == 0 and s.accounted()
    assert sorted(s.dirty) == [0, sizes[-1]]


def test_failed_launch_in_a_scoped_pass():
    s = _Sim()
    _pass(s, 32)
    with pytest.raises(RuntimeError, match="launch failed"):
        with s.scoped(None, 64) as bufs:
            _stats(bufs, 64)                              # partial work: sums, but the other buffer is never cleared
            raise RuntimeError("launch failed")
    assert not s.accounted()                             # what the bookkeeping calls clean is not
    _pass(s, 64)
    _pass(s, 16)
    assert s.resets == 1 and s.accounted()


def test_failed_launch_in_one_call():
    s = _Sim()
    _pass(s, 32)
    with pytest.raises(RuntimeError, match="launch failed"):
        with s.one_call():
            bufs = [s.acquire(None, n) for n in (8, 16, 24)]
            _launch(bufs[0], 8)
            _stats(bufs[1], 16)
            raise RuntimeError("launch failed")
    _pass(s, 128)                                        # hold is back to 0: this eager acquire clears
    assert s.resets == 1 and s.accounted()


def test_one_call_on_a_poisoned_pair_clears_once_before_its_first_acquire():
    """The block driver hands out every layer's buffers before its first launch: a clear at the second or third acquire would
    declare a buffer clean that an earlier layer of the same call is about to fill (the NaN of test_hip_graphed_step that
    EXPERIMENTS.md records)."""
    s = _Sim()
    with pytest.raises(RuntimeError):
        with s.scoped(None, 64) as bufs:
            _stats(bufs, 64)
            raise RuntimeError("launch failed")
    for sizes in ((32, 64, 16), (16, 8, 128)):           # the second call: nothing is owed any more
        with s.one_call():
            bufs = [s.acquire(None, n) for n in sizes]
            assert s.resets == 1
            for b, n in zip(bufs, sizes):
                _launch(b, n)
    _pass(s, 8)
    assert s.resets == 1 and s.accounted()


def test_one_call_after_a_capture_clears_once():
    s = _Sim()
    s.cap = 3
    _pass(s, 16)
    s.cap = 0
    with s.one_call():
        bufs = [s.acquire(None, n) for n in (32, 64, 16)]
        for b, n in zip(bufs, (32, 64, 16)):
            _launch(b, n)
    assert s.resets == 2 and s.accounted()               # one in the capture, one for the whole eager call


def _link():
    return _BnLink(None, None, None, None, None, 0, 1, 8, 4)


def _produce(s, link, t, n=16):
    """A kernel that writes the gradient ``t`` takes ``link``'s statistics too; the clear is left to the layer's apply pass."""
    with s.scoped(None, n) as bufs:
        _stats(bufs, n)
    s.hand_off(link, t, *bufs)
    return bufs


def test_hand_off_and_take():
    s = _Sim()
    _pass(s, 32)
    link, t = _link(), torch.zeros(4)
    bufs = _produce(s, link, t)
    assert link.holds_sums()
    got = s.take(link, t)
    assert got is not None and all(a is b for a, b in zip(got, bufs))
    assert not link.holds_sums() and s.pending is None
    with s:
        _apply(got)
    _pass(s, 8)
    assert s.resets == 0 and s.accounted()


@pytest.mark.parametrize("how", ["other tensor", "version moved", "other layout"])
def test_take_with_a_gradient_the_sums_do_not_belong_to(how):
    s = _Sim()
    _pass(s, 32)
    link, t = _link(), torch.zeros(4)
    _produce(s, link, t)
    if how == "version moved":
        t.add_(1.0)
    assert s.take(link, torch.zeros(4) if how == "other tensor" else t, how != "other layout") is None
    assert not link.holds_sums() and s.pending is None
    _pass(s, 64)                                         # the 32 doubles whose clear was deferred are gone by now
    _pass(s, 64)
    assert s.resets == 1 and s.accounted()


def test_an_acquire_between_hand_off_and_take_drops_the_sums():
    s = _Sim()
    _pass(s, 32)
    link, t = _link(), torch.zeros(4)
    _produce(s, link, t)
    _pass(s, 64)                                         # another BN backward node ran first
    assert s.resets == 1 and not link.holds_sums() and s.pending is None
    assert s.take(link, t) is None                       # nothing was left: the layer runs its own statistics pass ...
    _pass(s, 16)
    assert s.resets == 1 and s.accounted()               # ... and nothing more is owed


def test_take_from_a_link_without_sums_changes_nothing():
    s = _Sim()
    assert s.take(_link(), torch.zeros(4)) is None
    _pass(s, 8)
    assert s.resets == 0 and s.accounted()


def test_capture_resets_once_and_every_eager_call_afterwards_resets():
    s = _Sim()
    _pass(s, 32)
    s.cap = 7
    _pass(s, 16)
    assert s.resets == 1
    _pass(s, 16)
    _pass(s, 64)
    assert s.resets == 1                                 # the same capture: once
    s.cap = 8
    _pass(s, 16)
    assert s.resets == 2                                 # a new capture
    s.cap = 0
    for k in range(3):
        _pass(s, 24)
        assert s.resets == 3 + k                         # a replay may have run since: every eager call starts clean
    assert s.accounted()


def test_fold_reset_hands_the_store_out_once_per_capture():
    s = _Sim()
    _pass(s, 32)
    link, t = _link(), torch.zeros(4)
    _produce(s, link, t)
    assert s.fold_reset(0) is None                       # not capturing
    st = s.fold_reset(9)
    assert st is s.store and not link.holds_sums() and s.pending is None
    st.zero_()                                           # the weight-plane refresh clears it in its own launch
    assert s.fold_reset(9) is None
    s.cap = 9
    _pass(s, 16)
    _pass(s, 48)
    assert s.resets == 0 and s.accounted()
    assert s.fold_reset(10) is s.store


def test_a_changed_stream_waits_for_the_previous_one_once():
    s = _Sim()
    _pass(s, 16)
    _pass(s, 16)
    assert s.waits == []                                 # the first caller and the same stream: nothing to wait for
    s.raw = 2
    _pass(s, 16)
    _pass(s, 16)
    assert s.waits == [(2, 1)]
    s.raw = 1
    _pass(s, 16)
    assert s.waits == [(2, 1), (1, 2)] and s.resets == 0 and s.accounted()


def test_fits():
    assert _BnScratch.fits(_BnScratch.DOUBLES) and not _BnScratch.fits(_BnScratch.DOUBLES + 1)
    assert _BnScratch.existing(torch.device("cpu")) is None          # a test instance is never registered
