"""The BatchNorm passes of the composed path, host side: every Python call of a ``gkg_bn_*`` entry point (and of
gkg_nchw_to_tm_add_bnstats) and the record those calls read a layer from — ``bn_scratch._BnLink``: (Y, a, c, mean, invstd), (act, nb,
co, R), the statistics exchange ``sync`` and, for a layer on its running statistics, ``(bn, bias)``.

Mechanism only.  Which sequence a layer takes is decided in ``fused.py`` (its switches and predicates: _sync_group, _derive_ok,
_bn_scale_in_kernel, _bwd_fuse_ok, _bn_link) and arrives as arguments — the statistics ``group`` of a forward (None: rank-local), the
``atomic`` flag of a backward (the fp64-atomic two-launch form on the scratch pair; else the two-stage workspace form) — so this
module reads no switch and does not import ``fused``.  The block driver (``block.py``) issues the same passes from C; it takes the
mode predicates and the running-statistics helper from here."""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import _lib, derived
from .bn_scratch import _BnScratch
from .ops import _ptr, _stream

_F32 = torch.float32


# ---- a BN module's mode, each fact spelled once (whether a forward updates the running statistics: touch, below)
def batch_stats(bn) -> bool:
    """Normalises with the statistics of the batch (training, or a module that keeps no running statistics)."""
    return bn.training or not bn.track_running_stats


def frozen(bn) -> bool:
    """Normalises with its running statistics and does not update them (eval mode, statistics present)."""
    return not bn.training and bool(bn.track_running_stats) and bn.running_mean is not None and bn.running_var is not None


# ---- the running statistics of one call
def stats_ptrs(bn, track):
    """(running_mean, running_var, num_batches_tracked) as the entry points take them: pointers, or None x 3 when not tracked."""
    return (_ptr(bn.running_mean), _ptr(bn.running_var), _ptr(bn.num_batches_tracked)) if track else (None, None, None)


def touch(bn):
    """The kernels about to run update bn's running statistics through raw pointers: invalidate what was derived from them
    (layers._StatsEpoch) -> whether they do."""
    track = bn.training and bn.track_running_stats
    if track and hasattr(bn, "_gkg_epoch"):
        bn._gkg_epoch += 1
    return track


def running_stats(bn):
    """touch + stats_ptrs: what a train-mode pass hands its kernel."""
    return stats_ptrs(bn, touch(bn))


def _ws(lib, R, C, nb, device) -> torch.Tensor:
    """Workspace of the two-stage (deterministic) reductions."""
    return torch.empty(max(int(lib.gkg_bn_workspace_bytes(R, C, nb)), 256), dtype=torch.uint8, device=device)


# ---- forward
def eval_ac(lib, bn, bias, n):
    """(a, c) of an eval-mode BN folded with the conv bias: out = a*Y + c.  One small kernel, kept between calls (derived.get) —
    an inference forward launched it per layer —, never with gradients on."""
    def build():
        a = torch.empty(n, dtype=_F32, device=bn.weight.device)
        c = torch.empty_like(a)
        _lib.check(lib.gkg_bn_eval_affine(_ptr(bn.weight), _ptr(bn.bias), _ptr(bias), _ptr(bn.running_mean),
                                          _ptr(bn.running_var), _ptr(a), _ptr(c), n, float(bn.eps), _stream()),
                   "gkg_bn_eval_affine")
        return a, c
    srcs = (bn.weight, bn.bias, bn.running_mean, bn.running_var) + (() if bias is None else (bias,))
    return derived.get(bn, "eval_ac", srcs, build, extra=(bn.eps, n), stats_of=bn, cacheable=not torch.is_grad_enabled())


def forward_params(lib, Y, bn, bias, R, C, nb, group):
    """Returns (a, c, mean, invstd, sync) for out = a*Y + c; updates running statistics in train mode.
    ``sync`` is None (local statistics) or (group, count): the statistics were summed over the ranks of ``group``
    (one all-reduce of the column sums, sums of squares and the row count) and ``count`` is the device scalar
    holding the total number of rows — the backward needs both."""
    if not batch_stats(bn):
        return eval_ac(lib, bn, bias, nb * C) + (None, None, None)
    dev = Y.device
    a, c, mean, invstd = (torch.empty(nb * C, dtype=_F32, device=dev) for _ in range(4))
    ws = _ws(lib, R, C, nb, dev)
    rm, rv, nbt = running_stats(bn)
    affine = (_ptr(bn.weight), _ptr(bn.bias), _ptr(bias), rm, rv, _ptr(a), _ptr(c), _ptr(mean), _ptr(invstd))
    if group is None:
        _lib.check(lib.gkg_bn_train_stats(_ptr(Y), *affine, R, C, nb, float(bn.momentum), float(bn.eps), nbt, _ptr(ws), ws.numel(),
                                          _stream()), "gkg_bn_train_stats")
        return a, c, mean, invstd, None
    buf = torch.empty(nb * 2 * C + 1, dtype=_F32, device=dev)              # [sums | row count]
    _lib.check(lib.gkg_bn_stats_sums(_ptr(Y), _ptr(buf), R, C, nb, _ptr(ws), ws.numel(), _stream()), "gkg_bn_stats_sums")
    count = buf[-1:]
    count.fill_(float(R))
    dist.all_reduce(buf, group=group)
    _lib.check(lib.gkg_bn_finalize(_ptr(buf), _ptr(count), *affine, C, nb, float(bn.momentum), float(bn.eps), nbt, _stream()),
               "gkg_bn_finalize")
    return a, c, mean, invstd, (group, count)


def apply_from_sums(lib, Y, sums, bn, bias, group, dims, dest, out_tm=None, prep=None):
    """BN-apply straight from the fp64 column sums the projection's epilogue left in the scratch pair (``sums`` = what
    _BnScratch.scoped gave: the caller issues projection and this pass inside that scope) -> (a, c, mean, invstd, sync).
    ``dims`` = (R, cout, nb) of Y.  ``dest`` = (res, out, ldo, obs, ochunk, act, nchw_B, scale, rows_per_scale): where act(BN(Y))
    (+ res) is stored — ``out`` with row pitch ``ldo``, batch stride ``obs`` and XM chunking ``ochunk``, or (``nchw_B`` images)
    channel-major —, ``scale`` / ``rows_per_scale`` the DropPath factor per image.  Three forms with one head and one tail: into
    ``dest``; ``out_tm``: channel-major AND token-major result, residual token-major (_dual);
    ``prep`` (a KnnProblem): the pass is also the k-NN's token preparation, whose workspace is allocated now, by the call that is a
    producer (a label block's fc1 finds the one its keys already live in).
    A statistics ``group``: ONE fp64 all-reduce in front — the sums and, in the double behind them, the row count — and the _sync
    forms, which divide by the exchanged count; ``sync`` = (group, count as an fp32 device scalar) for the backward."""
    cur, other, zero = sums
    R, cout, nb = dims
    res, out, ldo, obs, ochunk, act, nchw_B, scale, rows_per_scale = dest
    dev, n = Y.device, 2 * nb * cout
    a, c, mean, invstd = torch.empty((4, nb * cout), dtype=_F32, device=dev).unbind(0)     # one allocation
    head = (_ptr(Y), _ptr(cur), _ptr(bn.weight), _ptr(bn.bias), _ptr(bias), *running_stats(bn), _ptr(a), _ptr(c), _ptr(mean),
            _ptr(invstd))
    sfx, tail, sync = "", (float(bn.momentum), float(bn.eps), _ptr(other), zero), None
    if group is not None:
        cur[n:n + 1].fill_(float(R))
        dist.all_reduce(cur[:n + 1], group=group)
        count = torch.empty(1, dtype=_F32, device=dev)
        sfx, tail, sync = "_sync", tail + (cur.data_ptr() + 8 * n, _ptr(count)), (group, count)
    if prep is not None:
        name, mid = "gkg_bn_apply_knn_prep", prep.producer_args(lib, out, out_tm, res, ldo, ochunk)
    elif out_tm is not None:
        name, mid = "gkg_bn_apply_train_dual", (_ptr(res), _ptr(out), _ptr(out_tm), nchw_B, cout, R // nchw_B)
    else:
        name, mid = "gkg_bn_apply_train", (_ptr(res), _ptr(out), R, cout, nb, ldo, obs, ochunk, act, nchw_B, _ptr(scale),
                                           rows_per_scale)
    _lib.check(getattr(lib, name + sfx)(*head, *mid, *tail, _stream()), name + sfx)
    return a, c, mean, invstd, sync


# ---- backward
def relayout_bnstats(lib, dout_c, dtm_c, g, layer, B):
    """g (R, co) = dout_c (B, co, N)^T (+ dtm_c) with the BN backward statistics of  out = BN(layer.Y)  taken in the same pass;
    they are left on ``layer``, whose backward then runs the apply pass only."""
    scratch = _BnScratch.of(g.device)
    with scratch.scoped(lib, 2 * layer.co) as (cur, other, zero):
        _lib.check(lib.gkg_nchw_to_tm_add_bnstats(_ptr(dout_c), _ptr(dtm_c), _ptr(g), _ptr(layer.Y), _ptr(layer.mean),
                                                  _ptr(layer.invstd), _ptr(cur), B, layer.co, layer.R // B, _stream()),
                   "gkg_nchw_to_tm_add_bnstats")
    scratch.hand_off(layer, g, cur, other, zero)


def backward(lib, layer, g, ldg, g_bstride, dY, grads, want, row_scale, atomic):
    """The BN backward of a layer's autograd node, train or eval mode: dY from the upstream gradient ``g`` (row pitch / batch stride
    ``ldg`` / ``g_bstride``) -> (dbias, dgamma, dbeta) to return.  ``grads``: the (dgamma, dbeta) output tensors; ``want``: whether
    the conv bias, gamma and beta need a gradient (eval mode computes only those; a conv bias in front of train-mode BN has exactly
    zero gradient — BN removes the mean —: not materialised); ``row_scale`` = (factor per image, rows per image) or None: DropPath,
    applied by the kernels (eval mode and the atomic form take it)."""
    L, dev = layer, layer.Y.device
    rs, rps = (None, 0) if row_scale is None else (_ptr(row_scale[0]), row_scale[1])
    geom = (L.R, L.co, L.nb, ldg, g_bstride, L.act)
    dgamma, dbeta = grads
    if L.mean is None:
        return _eval_backward(lib, L, g, dY, geom, (rs, rps), (dgamma if want[1] else None, dbeta if want[2] else None),
                              want[0], atomic)
    head = (_ptr(g), _ptr(L.Y), _ptr(L.a), _ptr(L.c), _ptr(L.mean), _ptr(L.invstd))
    outs = (_ptr(dY), _ptr(dgamma), _ptr(dbeta))
    if L.holds_sums():
        # the kernel that wrote g also took this layer's statistics (dgrad epilogue, re-layout pass, aggregation scatter): when
        # they describe exactly this gradient tensor, only the apply pass runs
        scratch = _BnScratch.of(dev)
        sums = scratch.take(L, g, g_bstride == (L.co if L.nb > 1 else 0) and ldg == L.nb * L.co)
        if sums is not None:
            with scratch:
                _lib.check(lib.gkg_bn_bwd_apply_from_sums(*head, *outs, *geom, _ptr(sums[0]), _ptr(sums[1]), sums[2], _stream()),
                           "gkg_bn_bwd_apply_from_sums")
            return None, dgamma, dbeta
    n = 2 * L.nb * L.co
    if atomic:
        # two launches: statistics with fp64 atomics into one of two alternating scratch buffers, apply (which also clears
        # what the previous call left in the other buffer) — no partial rows, no second-stage reduction launch
        with _BnScratch.of(dev).scoped(lib, n) as (cur, other, zero):
            pair = (_ptr(cur), _ptr(other), zero)
            if L.sync is not None:
                # the same two launches with the exchange in the middle: this rank's sums are kept (dgamma / dbeta), the fp64
                # buffer itself is all-reduced, the apply pass divides by the exchanged row count
                group, count = L.sync
                _lib.check(lib.gkg_bn_bwd_stats_f64(*head, *geom, _ptr(cur), rs, rps, _stream()), "gkg_bn_bwd_stats_f64")
                local = cur[:n].clone()
                dist.all_reduce(cur[:n], group=group)
                _lib.check(lib.gkg_bn_bwd_apply_sync(*head, *outs, *geom, _ptr(local), _ptr(cur), _ptr(count), _ptr(other), zero,
                                                     rs, rps, _stream()), "gkg_bn_bwd_apply_sync")
            elif row_scale is not None:
                _lib.check(lib.gkg_bn_bwd_atomic_scaled(*head, *outs, *geom, *pair, rs, rps, _stream()), "gkg_bn_bwd_atomic_scaled")
            else:
                _lib.check(lib.gkg_bn_bwd_atomic(*head, *outs, *geom, *pair, _stream()), "gkg_bn_bwd_atomic")
        return None, dgamma, dbeta
    # two-stage form (GKG_DETERMINISTIC, or exchanged statistics off the x6 path: the sums travel as fp32 between its halves)
    ws = _ws(lib, L.R, L.co, L.nb, dev)
    if L.sync is None:
        _lib.check(lib.gkg_bn_bwd(*head, *outs, *geom, _ptr(ws), ws.numel(), _stream()), "gkg_bn_bwd")
        return None, dgamma, dbeta
    group, count = L.sync
    sums = torch.empty(n, dtype=_F32, device=dev)
    _lib.check(lib.gkg_bn_bwd_sums(*head, _ptr(dY), _ptr(sums), _ptr(dgamma), _ptr(dbeta), *geom, _ptr(ws), ws.numel(), _stream()),
               "gkg_bn_bwd_sums")
    dist.all_reduce(sums, group=group)
    _lib.check(lib.gkg_bn_bwd_apply(*head, _ptr(sums), _ptr(count), _ptr(dY), *geom, _stream()), "gkg_bn_bwd_apply")
    return None, dgamma, dbeta


def _eval_backward(lib, L, g, dY, geom, scale, grads, want_bias, atomic):
    """dY of out = act(BN_eval(Y)) (running statistics: a frozen BN, or a module in eval() with gradients) in ONE sweep
    (gkg_bn_eval_bwd) -> (dbias, dgamma, dbeta).  ``grads``: (dgamma, dbeta) outputs, None where not wanted — with any of the three
    the sweep also takes the two column sums (fp64 atomics into the alternating scratch pair, or the two-stage workspace form
    when not ``atomic``) and a small second launch finishes them; with none (a fully frozen affine) the pass is purely elementwise.
    ``dbias`` is the gradient of the conv bias in front of the BN: real here, exactly zero in train mode."""
    dgamma, dbeta = grads
    dev = L.Y.device
    dbias = torch.empty(L.nb * L.co, dtype=_F32, device=dev) if (L.bias is not None and want_bias) else None
    args = (_ptr(g), _ptr(L.Y), _ptr(L.a), _ptr(L.c), _ptr(dY), *geom, *scale, _ptr(L.bn.running_mean), _ptr(L.bn.running_var),
            _ptr(L.bias), float(L.bn.eps), _ptr(dgamma), _ptr(dbeta), _ptr(dbias))
    if dgamma is None and dbeta is None and dbias is None:
        _lib.check(lib.gkg_bn_eval_bwd(*args, None, None, 0, None, 0, _stream()), "gkg_bn_eval_bwd")
    elif atomic:
        with _BnScratch.of(dev).scoped(lib, 2 * L.nb * L.co) as (cur, other, zero):
            _lib.check(lib.gkg_bn_eval_bwd(*args, _ptr(cur), _ptr(other), zero, None, 0, _stream()), "gkg_bn_eval_bwd")
    else:
        ws = _ws(lib, L.R, L.co, L.nb, dev)
        _lib.check(lib.gkg_bn_eval_bwd(*args, None, None, 0, _ptr(ws), ws.numel(), _stream()), "gkg_bn_eval_bwd")
    return dbias, dgamma, dbeta
