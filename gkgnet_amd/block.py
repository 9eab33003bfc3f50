"""Block-level host side (round 6): a Grapher / GrapherLabel block's forward and backward as ONE library call each
(csrc/gkg_block.hip: gkg_grapher_fwd / _bwd, gkg_grapher_label_fwd / _bwd; reference torch_vertex.py:325-333, :392-403).

``fused.py`` composes a block from per-layer autograd Functions (≈ 25 ctypes calls and ≈ 1 800 Python calls per block pair and
step): right for the whole-backbone steps, which are GPU-bound, and host-bound for the small blocks an eager training loop launches
one by one.  Here the host allocates two arenas (what the forward saves, what the backward needs), fills a descriptor of pointers
and sizes and makes one call; the C side issues the same launches with the same arguments, so the results are bit-identical to the
composition (tests/test_hip_block_driver.py).  Taken automatically for the form the metric is quoted on — fp32, train-mode
BatchNorm with rank-local statistics, no DropPath scaling, un-pooled keys, every projection on the split-bf16 kernels, blocks
below the BN-epilogue row count — and for the same block with EVERY BatchNorm frozen (eval mode with running statistics:
``layers.freeze_batchnorm``, ``norm_eval``, ``eval()`` with gradients; a frozen SyncBatchNorm too): the descriptor's ``bn_frozen``
form, which writes no statistics and returns the conv biases' gradients (tests/test_hip_frozen_block_driver.py).  A block with
some layers frozen and some not, and everything else, keeps the composition.  GKG_DISABLE=block_driver: off.

Structure: a per-module ``_Plan`` holds what is the same on every step — the projections, the static half of the descriptor, and
the two arena layouts, which are data (``_ARENAS``: descriptor field -> size) resolved to (field, offset) pairs when the plan is
built.  The two autograd Functions keep what is their own (inputs, outputs, the Grapher's keys handshake and dual output, the label
block's announcement to its producer); everything a call shares lives once, in ``_forward`` and ``_backward``, which treat the
projections as a list in the plan's order (train: three autograd inputs each, frozen: four) — one ``_proj_fwd`` / ``_proj_bwd`` per
projection, whatever the mode.  The prepared-token handshake with the k-NN (problem, workspace, marks) is ``knn_prep.py``'s."""
from __future__ import annotations

import ctypes as C
import weakref
from contextlib import nullcontext

import torch

from . import _abi, _lib, bn_passes, fused, knn_prep
from .ops import _ptr, _stream

_F32 = torch.float32
# The block entry points' descriptors: include/gkg_hip.h's structs as _abi.py derives them (fields in declaration order).
_S = _abi.header().structs
ProjBN, GraphOp, GrapherBlock, LabelBlock = _S["GkgProjBN"], _S["GkgGraphOp"], _S["GkgGrapherBlock"], _S["GkgLabelBlock"]

ENABLED = "block_driver" not in fused._DISABLED


# ----------------------------------------------------------------------------------------------- eligibility
def _proj_ok(seq, R, cin, cout, nb, frozen=False) -> bool:
    """One projection + BN in the driver's scope, in train mode or (``frozen``) on its running statistics."""
    conv, bn = seq[0], seq[1]
    if not (conv.weight.dtype == _F32 and bn.weight.dtype == _F32 and fused._bn_ok(bn) and fused._sync_group(bn) is None
            and isinstance(bn, torch.nn.modules.batchnorm._BatchNorm) and fused._x6_rule(R, cin, cout, nb, "fwd")
            and (conv.bias is None or conv.bias.dtype == _F32)):
        return False
    if frozen:
        return (bn_passes.frozen(bn) and bn.running_mean.dtype == _F32 and bn.running_var.dtype == _F32
                and fused._BnScratch.fits(2 * nb * cout))
    return bn.training and fused._derive_ok(bn, nb, cout, _lib.F32, False)


def _block_mode(bn):
    """The mode every projection of a block must share, read off its first BN: True frozen, False train, None neither."""
    if bn.training:
        return False
    return True if bn_passes.frozen(bn) else None


def _common_ok(x) -> bool:
    return (ENABLED and fused.ENABLED and fused.GEMM_MATH == "x6" and not fused.DETERMINISTIC and fused.XM_DIRECT
            and x.is_cuda and x.dtype == _F32 and not torch.is_autocast_enabled() and torch.is_grad_enabled()
            and fused.knn_graph_tm is fused._KNN_GRAPH_TM)


def _drops(dp) -> bool:
    """An ACTIVE DropPath (asked without drawing: the eligibility test must not consume random numbers)."""
    if hasattr(dp, "active"):
        return bool(dp.active())
    return not isinstance(dp, torch.nn.Identity)


def grapher_ok(mod, x, relative_pos, groups, want_edge, dual) -> bool:
    """The block driver applies to this Grapher call (see the module docstring); ``fused.grapher_forward`` asks."""
    if not _common_ok(x) or want_edge or x.dim() != 4 or fused.is_channels_last(x):
        return False
    gc = mod.graph_conv
    B, Cc, H, W = x.shape
    T = B * H * W
    nn_ = gc.gconv.nn
    if (gc.r != 1 or Cc % 16 or (Cc // groups) % 4 or T >= fused.BN_EPILOGUE_MIN_ROWS or len(nn_) != 3
            or _drops(mod.drop_path) or H * W > 65536):
        return False
    fz = _block_mode(mod.fc1[1])
    if fz is None or not (_proj_ok(mod.fc1, T, Cc, Cc, 1, fz) and _proj_ok(nn_, T, Cc // 2, Cc // 2, 4, fz)
                          and _proj_ok(mod.fc2, T, 2 * Cc, Cc, 1, fz)):
        return False
    if nn_[0].groups != 4 or tuple(nn_[0].weight.shape[:2]) != (2 * Cc, Cc // 2) or not isinstance(nn_[2], torch.nn.GELU):
        return False
    fm = fused._knn_mr_shapes_ok(B, H * W, Cc, H * W, False, relative_pos, gc.k, gc.d, groups, nn_, False)
    return bool(fm or fused.KNN_COMPACT)


def label_ok(mod, e, ft, groups) -> bool:
    if not _common_ok(e) or ft.dtype != _F32 or not ft.is_contiguous():
        return False
    gc = mod.graph_conv
    B, L, Cc = e.shape
    T = B * L
    M = ft.shape[1]
    nn_ = gc.gconv.nn
    Cf = mod.ffn.fc1[0].weight.shape[0]
    if (Cc % 16 or (Cc // groups) % 4 or T >= fused.BN_EPILOGUE_MIN_ROWS or len(nn_) != 3 or M > 65536
            or _drops(mod.drop_path) or _drops(mod.ffn.drop_path)
            or not isinstance(mod.ffn.act, torch.nn.GELU) or not isinstance(nn_[2], torch.nn.GELU)):
        return False
    if nn_[0].groups != 4 or tuple(nn_[0].weight.shape[:2]) != (2 * Cc, Cc // 2):
        return False
    fz = _block_mode(mod.fc1[1])
    return (fz is not None and _proj_ok(mod.fc1, T, Cc, Cc, 1, fz) and _proj_ok(nn_, T, Cc // 2, Cc // 2, 4, fz)
            and _proj_ok(mod.fc2, T, 2 * Cc, Cc, 1, fz) and _proj_ok(mod.ffn.fc1, T, Cc, Cf, 1, fz)
            and _proj_ok(mod.ffn.fc2, T, Cf, Cc, 1, fz))


# ----------------------------------------------------------------------------------------------- plans
# What a block call needs to know about its module is the same on every step: which tensors the five projections read, their
# sizes, the layout of the two arenas, the static half of the descriptor.  A _Plan holds it (built on the first eligible call,
# through the full eligibility test above) and a per-call guard that is a few dozen identity / pointer comparisons; Grapher.forward
# and GrapherLabel.forward ask try_grapher / try_label first and reach the C entry point after ~40 us of Python instead of ~150.
_PLANS = weakref.WeakKeyDictionary()           # module -> {(shape key, switches): _Plan}


def _switches():
    return (ENABLED, fused.ENABLED, fused.GEMM_MATH, fused.DETERMINISTIC, fused.XM_DIRECT, fused.KNN_MR, fused.KNN_COMPACT,
            fused.KNN_PREP, fused.KNN_BF16, fused.KNN_F16, fused.BN_EPILOGUE_MIN_ROWS, fused.knn_graph_tm is fused._KNN_GRAPH_TM)


class _Proj:
    """One 1x1 projection + BN of a block: the tensors its kernels read through raw pointers, and its sizes."""
    __slots__ = ("conv", "bn", "W", "bias", "gamma", "beta", "rm", "rv", "nbt", "nb", "cin", "cout", "kperm", "trs", "mom", "eps",
                 "wshape", "nch", "wreal")

    def __init__(self, seq, nb, cin, cout, kperm, wshape, ident):
        conv, bn = seq[0], seq[1]
        self.conv, self.bn = conv, bn
        self.W, self.bias, self.gamma, self.beta = conv.weight, conv.bias, bn.weight, bn.bias
        self.trs = bool(bn.track_running_stats)
        self.rm, self.rv, self.nbt = bn.running_mean, bn.running_var, bn.num_batches_tracked
        self.nb, self.cin, self.cout, self.kperm = nb, cin, cout, kperm
        self.mom, self.eps = bn.momentum, bn.eps
        self.wshape, self.nch, self.wreal = wshape, nb * cout, conv.weight.shape
        ident += [(seq._modules, "0", conv), (seq._modules, "1", bn), (conv._parameters, "weight", self.W),
                  (conv._parameters, "bias", self.bias), (bn._parameters, "weight", self.gamma), (bn._parameters, "bias", self.beta),
                  (bn._buffers, "running_mean", self.rm), (bn._buffers, "running_var", self.rv),
                  (bn._buffers, "num_batches_tracked", self.nbt)]

    def static(self, p: ProjBN):
        p.gamma, p.beta, p.bias = _ptr(self.gamma), _ptr(self.beta), _ptr(self.bias)
        p.running_mean, p.running_var, p.nbt = bn_passes.stats_ptrs(self.bn, self.trs)
        p.momentum, p.eps = float(self.mom), float(self.eps)
        p.cin, p.cout, p.nb = self.cin, self.cout, self.nb

    def baked(self):
        return [t for t in (self.gamma, self.beta, self.bias) + ((self.rm, self.rv, self.nbt) if self.trs else ()) if t is not None]


# The two arenas of a block call — what the forward saves, what the backward needs — as data: per block kind the descriptor fields
# that point into the arena, in arena order, each with its size in fp32 elements as rows x columns (T tokens, C channels, Cf the
# FFN's width; `fc1.Y` is field Y of the projection fc1; a BN's `bn` holds a, c, mean, invstd per channel — the grouped projection
# has 4 x C/2 channels —, `graph.arg` the u16 winning rows).  A piece starts 16-byte aligned.
_ARENAS = {
    "g": ((("xt", "T", "C"), ("XM", "T", "2C"), ("A2", "T", "2C"), ("fc1.Y", "T", "C"), ("conv.Y", "T", "2C"), ("fc2.Y", "T", "C"),
           ("fc1.bn", "4", "C"), ("conv.bn", "4", "2C"), ("fc2.bn", "4", "C"), ("graph.arg", "T", "C/2")),
          (("g3", "T", "C"), ("dY3", "T", "C"), ("gx1", "T", "C"), ("dY1", "T", "C"), ("dxt", "T", "C"), ("dA2", "T", "2C"),
           ("dY2", "T", "2C"), ("dXM", "T", "2C"))),
    "l": ((("XM", "T", "2C"), ("A2", "T", "2C"), ("h2", "T", "C"), ("f1", "T", "Cf"), ("fc1.Y", "T", "C"), ("conv.Y", "T", "2C"),
           ("fc2.Y", "T", "C"), ("ffn1.Y", "T", "Cf"), ("ffn2.Y", "T", "C"), ("fc1.bn", "4", "C"), ("conv.bn", "4", "2C"),
           ("fc2.bn", "4", "C"), ("ffn1.bn", "4", "Cf"), ("ffn2.bn", "4", "C"), ("graph.arg", "T", "C/2")),
          (("dY5", "T", "C"), ("dh2", "T", "C"), ("dY3", "T", "C"), ("gx1", "T", "C"), ("dY1", "T", "C"), ("df1", "T", "Cf"),
           ("dY4", "T", "Cf"), ("dA2", "T", "2C"), ("dY2", "T", "2C"), ("dXM", "T", "2C"))),
}


def _layout(table, T, Cc, Cf):
    """One arena of _ARENAS for these sizes -> (((sub-structure | None, ((field, byte offset), ...)), ...), total elements): the
    names resolved here, once per plan, so that a call only stores pointers (_point)."""
    dim = {"T": T, "4": 4, "C": Cc, "2C": 2 * Cc, "C/2": Cc // 2, "Cf": Cf}
    owners, o = {}, 0
    for path, rows, cols in table:
        owner, _, field = path.rpartition(".")
        owners.setdefault(owner or None, []).append((field, 4 * o))
        o += (dim[rows] * dim[cols] + 3) & ~3
    return tuple((owner, tuple(fields)) for owner, fields in owners.items()), o


def _point(d, arena, base):
    """Point the descriptor's fields of one arena (_layout) into the buffer at ``base``."""
    for owner, fields in arena:
        obj = d if owner is None else getattr(d, owner)
        for field, off in fields:
            setattr(obj, field, base + off)


class _Plan:
    __slots__ = ("kind", "projs", "ident", "tensors", "ptrs", "tmpl", "names", "stride", "fwd", "fwd_total", "bwd", "bwd_total", "drops",
                 "sync", "gc", "nn_", "k", "d", "groups", "dims", "rp", "rp_view", "fast", "params", "fm", "has_bucket", "frozen",
                 "gelus", "__weakref__")

    def valid(self) -> bool:
        for dct, key, obj in self.ident:
            if dct.get(key) is not obj:
                return False
        frozen = self.frozen
        for p in self.projs:
            bn = p.bn
            # (the recorded mode: a BN switched in either direction drops the plan; the tensors behind a frozen layer's running
            # statistics are among self.ident / self.tensors)
            if (bn.training == frozen or bn.track_running_stats != p.trs or bn.momentum != p.mom or bn.eps != p.eps
                    or not bn.affine or p.W.shape != p.wreal or p.W.dtype != _F32):
                return False
        if self.ptrs != [t.data_ptr() for t in self.tensors]:
            return False
        for dp in self.drops:
            if _drops(dp):
                return False
        gc = self.gc
        if gc.k != self.k or gc.d != self.d or gc.r != 1 or getattr(gc.dilated_knn_graph, "stochastic", False):
            return False
        if self.nn_[0].groups != 4:
            return False
        for m in self.gelus():
            if not isinstance(m, torch.nn.GELU):
                return False
        if self.sync:
            for p in self.projs:
                if fused._sync_group(p.bn) is not None:
                    return False
        return True


def _finish_plan(plan, mod, cls, projs, ident, drops, gc, nn_, groups, dims, relative_pos, T, Cc, Cf):
    plan.projs, plan.ident, plan.drops, plan.gc, plan.nn_, plan.groups, plan.dims = projs, ident, drops, gc, nn_, groups, dims
    plan.k, plan.d = gc.k, gc.d
    plan.frozen = not projs[0].bn.training                 # (grapher_ok / label_ok: every projection in the same mode)
    ffn = mod._modules.get("ffn")
    plan.gelus = (lambda: (nn_[2],)) if ffn is None else (lambda: (nn_[2], ffn.act))
    plan.tensors = [t for p in projs for t in p.baked()]
    plan.ptrs = [t.data_ptr() for t in plan.tensors]
    plan.sync = any(isinstance(p.bn, torch.nn.SyncBatchNorm) for p in projs)
    fwd, bwd = _ARENAS[plan.kind]
    plan.fwd, plan.fwd_total = _layout(fwd, T, Cc, Cf)
    plan.bwd, plan.bwd_total = _layout(bwd, T, Cc, Cf)
    # the autograd inputs, `stride` per projection: a conv bias in front of a frozen BN has a real gradient (in train mode it is
    # exactly zero: no input)
    plan.stride = 4 if plan.frozen else 3
    plan.params = tuple(t for p in projs for t in (p.W, p.gamma, p.beta, p.bias)[:plan.stride])
    plan.fm = {}
    own = mod._parameters.get("relative_pos", mod.__dict__.get("relative_pos"))
    plan.fast = relative_pos is None or relative_pos is own        # a re-interpolated bias is a new tensor every call: slow path
    plan.rp = relative_pos if plan.fast else None                  # (a slow plan must not keep that call's tensor alive)
    plan.rp_view = None
    if relative_pos is not None and plan.fast:
        ident.append((mod._parameters, "relative_pos", relative_pos))
    d = cls()
    d.bn_frozen = int(plan.frozen)
    plan.names = tuple(f[0] for f in cls._fields_ if f[1] is ProjBN)          # the projections' descriptor fields, in forward order
    for nm, p in zip(plan.names, projs):
        p.static(getattr(d, nm))
    plan.tmpl = bytes(d)
    return plan


def _plan_grapher(mod, x, relative_pos, groups):
    plans = _PLANS.setdefault(mod, {})
    key = ("g", tuple(x.shape), groups, _switches())
    plan = plans.get(key)
    if plan is not None and plan.valid() and (plan.rp is relative_pos or not plan.fast):
        return plan
    B, Cc, H, W = x.shape
    T = B * H * W
    gc = mod.graph_conv
    nn_ = gc.gconv.nn
    ident = [(mod._modules, "fc1", mod.fc1), (mod._modules, "fc2", mod.fc2), (mod._modules, "graph_conv", gc),
             (mod._modules, "drop_path", mod.drop_path), (gc._modules, "gconv", gc.gconv), (gc.gconv._modules, "nn", nn_)]
    projs = [_Proj(mod.fc1, 1, Cc, Cc, 0, (Cc, Cc), ident), _Proj(nn_, 4, Cc // 2, Cc // 2, 1, (4, Cc // 2, Cc // 2), ident),
             _Proj(mod.fc2, 1, 2 * Cc, Cc, 0, (Cc, 2 * Cc), ident)]
    plan = _Plan()
    plan.kind = "g"
    _finish_plan(plan, mod, GrapherBlock, projs, ident, [mod.drop_path], gc, nn_, groups, (B, Cc, H, W), relative_pos, T, Cc, 0)
    plans[key] = plan
    return plan


def _plan_label(mod, e2, ft, groups):
    plans = _PLANS.setdefault(mod, {})
    B, M, Cc = ft.shape
    T = e2.shape[0]
    key = ("l", T, tuple(ft.shape), groups, _switches())
    plan = plans.get(key)
    if plan is not None and plan.valid():
        return plan
    L = T // B
    gc = mod.graph_conv
    nn_ = gc.gconv.nn
    ffn = mod.ffn
    Cf = ffn.fc1[0].weight.shape[0]
    ident = [(mod._modules, "fc1", mod.fc1), (mod._modules, "fc2", mod.fc2), (mod._modules, "graph_conv", gc),
             (mod._modules, "drop_path", mod.drop_path), (mod._modules, "ffn", ffn), (ffn._modules, "fc1", ffn.fc1),
             (ffn._modules, "fc2", ffn.fc2), (ffn._modules, "drop_path", ffn.drop_path), (ffn._modules, "act", ffn.act),
             (gc._modules, "gconv", gc.gconv), (gc.gconv._modules, "nn", nn_)]
    projs = [_Proj(mod.fc1, 1, Cc, Cc, 0, (Cc, Cc), ident), _Proj(nn_, 4, Cc // 2, Cc // 2, 1, (4, Cc // 2, Cc // 2), ident),
             _Proj(mod.fc2, 1, 2 * Cc, Cc, 0, (Cc, 2 * Cc), ident), _Proj(ffn.fc1, 1, Cc, Cf, 0, (Cf, Cc), ident),
             _Proj(ffn.fc2, 1, Cf, Cc, 0, (Cc, Cf), ident)]
    plan = _Plan()
    plan.kind = "l"
    _finish_plan(plan, mod, LabelBlock, projs, ident, [mod.drop_path, ffn.drop_path], gc, nn_, groups, (B, Cc, L, M, Cf), None, T, Cc, Cf)
    plans[key] = plan
    return plan


# ----------------------------------------------------------------------------------------------- descriptor pieces
def _proj_fwd(lib, p: ProjBN, pr: _Proj, scratch, keep):
    """The per-call half of a projection's forward descriptor: weight planes (refreshed when the weight moved) and the BN pass's
    scratch buffers (Y and the BN coefficients live in the forward arena)."""
    pf, pd = fused._planes(lib, pr.W, pr.nb, pr.cout, pr.cin, True, True, kperm=pr.kperm)
    p.planes_fwd, p.planes_dgrad = pf.data_ptr(), pd.data_ptr()
    if scratch is not None:                                   # (None: a frozen layer — no statistics pass, nothing written back)
        bn_passes.touch(pr.bn)                                # the kernels update the running statistics
        cur, other, zero = scratch.acquire(lib, 2 * pr.nch)
        p.fsum, p.fzero, p.fzero_n = cur.data_ptr(), other.data_ptr(), zero
    keep.append(pf)
    keep.append(pd)


def _want_1d(need, projs) -> bool:
    """Whether a frozen block's backward computes any gamma / beta / conv-bias gradient (``need``: the needs_input_grad slice of
    its parameters, four per projection)."""
    return any(need[4 * i + 1] or need[4 * i + 2] or (need[4 * i + 3] and pr.bias is not None) for i, pr in enumerate(projs))


def _slot(param, n, dev):
    """Where a 1-D parameter gradient goes: the parameter's gradient-bucket slot, else a fresh tensor."""
    v = fused.grad_view(param, (n,)) if param.dtype == _F32 else None
    return torch.empty(n, dtype=_F32, device=dev) if v is None else v


def _proj_bwd(lib, p: ProjBN, pr: _Proj, scratch, dev, want):
    """Backward half of a projection's descriptor -> (dW, dgamma, dbeta, dbias): the gradient outputs (bucket slots when the
    parameters have them) and the BN pass's scratch buffers.  ``want`` None: train mode — gamma's and beta's gradients are always
    written, the conv bias has none, the scratch pair is always used.  A frozen layer passes ctx.needs_input_grad of (W, gamma,
    beta, bias): only the wanted 1-D gradients get a pointer (gkg_bn_eval_bwd computes those and nothing else), and the scratch
    pair is acquired only when there is one.  The weight gradient is always computed, like the composition's."""
    if want is None:
        dWv, dgamma, dbeta = fused._grad_outs((pr.W, pr.gamma, pr.beta), pr.wshape, pr.nch, dev)
        dbias = None
    else:
        wv = fused.grad_view(pr.W, pr.wshape) if pr.W.dtype == _F32 else None
        dWv = torch.empty(pr.wshape, dtype=_F32, device=dev) if wv is None else wv
        dgamma = _slot(pr.gamma, pr.nch, dev) if want[1] else None
        dbeta = _slot(pr.beta, pr.nch, dev) if want[2] else None
        dbias = _slot(pr.bias, pr.nch, dev) if (want[3] and pr.bias is not None) else None
    if not getattr(dWv, "_gkg_zero", False):
        dWv.zero_()                                      # the weight-gradient kernels ADD into dw
    if want is None or dgamma is not None or dbeta is not None or dbias is not None:
        cur, other, zero = scratch.acquire(lib, 2 * pr.nch)
        p.bsum, p.bzero, p.bzero_n = cur.data_ptr(), other.data_ptr(), zero
    else:
        p.bsum, p.bzero, p.bzero_n = None, None, 0
    p.dw, p.dgamma, p.dbeta, p.dbias = dWv.data_ptr(), _ptr(dgamma), _ptr(dbeta), _ptr(dbias)
    return dWv, dgamma, dbeta, dbias


def _graph_op(lib, plan, g: GraphOp, B, G, c, N, M, relative_pos, has_y, want_edge, dev, keys_key, keep):
    """The block's k-NN + aggregation: kernel form, flags, workspace (shared with a keys producer when the Grapher in front prepared
    this graph's keys).  -> (key object of this k-NN problem, edge tensor | None)."""
    k, d = plan.k, plan.d
    flags0 = knn_prep.problem_flags(relative_pos)            # (once per call: the kernel choice below is cached per flag word)
    fm = plan.fm.get(flags0)
    if fm is None:
        fm = plan.fm[flags0] = bool(fused._knn_mr_shapes_ok(B, N, G * c, M, has_y, relative_pos, k, d, G, plan.nn_, False))
    key = knn_prep.KnnProblem(B, G, c, N, M, k, d, has_y, relative_pos, fm, flags0)
    flags = flags0
    if fused.KNN_PREP:
        flags |= _lib.KNN_X_PREPARED                         # no tuple to match: this call's own fc1 step is the queries' producer
        if key.adopt_keys(keys_key):
            flags |= _lib.KNN_Y_PREPARED
    key.workspace(lib, dev)
    rp = None
    if relative_pos is not None:
        rp = plan.rp_view if relative_pos is plan.rp else None
        if rp is None or rp.data_ptr() != relative_pos.data_ptr():
            rp = fused._rp_arg(relative_pos, N, M)
            if relative_pos is plan.rp and plan.fast and rp.data_ptr() == relative_pos.data_ptr():
                plan.rp_view = rp                      # a reshaped view of the module's own parameter: the same view every call
    g.G, g.k, g.d, g.fused_mr = G, k, d, int(fm)
    g.relpos, g.knn_flags, g.mr_flags = _ptr(rp), flags, fused._mr_bwd_flags()
    g.knn_ws, g.knn_ws_bytes = key.ws.data_ptr(), key.ws.numel()
    edge = None
    if want_edge:
        edge = torch.empty((2, B * G, N, k), dtype=torch.int64, device=dev)
        g.nn_idx, g.center = edge[0].data_ptr(), edge[1].data_ptr()
    elif not fm:
        nn16 = torch.empty((B * G, N, k), dtype=torch.int16, device=dev)
        g.nn16 = nn16.data_ptr()
        keep.append(nn16)
    keep.append(rp)
    keep.append(key.ws)
    return key, edge


def _issue_wgrads(lib, wq, n, outs, keep, device):
    """The block's weight-gradient problems: into the backward pass's batched launch when every dW is a bucket slot (and a backward
    pass is running to flush it), else launched now."""
    if fused._wgrad_defer_block(wq, n, outs, keep, device):
        return
    _lib.check(lib.gkg_linear_wgrad_x6_batch(wq, n, fused.WGRAD_UNITS, _stream()), "gkg_linear_wgrad_x6_batch (block)")


# ----------------------------------------------------------------------------------------------- the two Functions' common part
def _forward(lib, plan, d, dev, N, M, relative_pos, has_y, want_edge, keys_key, entry):
    """A block's forward call on the descriptor ``d`` (a copy of the plan's template with the block's own inputs and outputs set):
    BN scratch (none for a frozen block: no statistics pass), forward arena, the projections, the graph op, the split-K workspace,
    the call -> (arena, key object of the k-NN problem, edge tensor | None)."""
    keep = []
    scratch = None if plan.frozen else fused._BnScratch.of(dev)
    buf = torch.empty(plan.fwd_total, dtype=_F32, device=dev)
    _point(d, plan.fwd, buf.data_ptr())
    B, Cc, groups = plan.dims[0], plan.dims[1], plan.groups
    with (nullcontext() if scratch is None else scratch.one_call()):
        for nm, pr in zip(plan.names, plan.projs):
            _proj_fwd(lib, getattr(d, nm), pr, scratch, keep)
        key, edge = _graph_op(lib, plan, d.graph, B, groups, Cc // groups, N, M, relative_pos, has_y, want_edge, dev, keys_key, keep)
        sk = fused._sk_ws(dev)
        d.sk_ws, d.sk_bytes = sk.data_ptr(), sk.numel()
        _lib.check(getattr(lib, entry)(C.byref(d), _stream()), entry)
    return buf, key, edge


def _backward(ctx, buf, weights, lead, keep, entry):
    """A block's backward call on ctx.desc (the block's own gradient inputs and outputs set): backward arena, flags, BN scratch
    (none for a frozen block that wants no 1-D gradient), the projections in backward order — the order of wq[] —, the call, the
    weight gradients -> ``lead`` (the gradients of the inputs in front of the parameters) + per projection, in forward order,
    (dW, dgamma, dbeta[, dbias])."""
    lib = _lib.load()
    plan, d, dev = ctx.plan, ctx.desc, buf.device
    tbuf = torch.empty(plan.bwd_total, dtype=_F32, device=dev)
    _point(d, plan.bwd, tbuf.data_ptr())
    d.bwd_flags = fused._block_flags()
    n, st = len(plan.projs), plan.stride
    need = ctx.needs_input_grad[len(lead):]
    scratch = fused._BnScratch.of(dev) if (not plan.frozen or _want_1d(need, plan.projs)) else None
    wq = (_lib.WgradProblem * n)()
    outs = [None] * n
    with (nullcontext() if scratch is None else scratch.one_call()):
        for i in reversed(range(n)):
            outs[i] = _proj_bwd(lib, getattr(d, plan.names[i]), plan.projs[i], scratch, dev,
                                need[st * i:st * (i + 1)] if plan.frozen else None)
        _lib.check(getattr(lib, entry)(C.byref(d), wq, _stream()), entry)
    _issue_wgrads(lib, wq, n, tuple(o[0] for o in reversed(outs)), (buf, tbuf) + keep, dev)
    grads = list(lead)
    for o, w in zip(outs, weights):
        grads.append(o[0].view_as(w))
        grads += o[1:st]
    return tuple(grads)


# ----------------------------------------------------------------------------------------------- Grapher
class _GrapherBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan, relative_pos, label_knn, dual, *params):
        # params: (W, gamma, beta) of fc1, the grouped projection and fc2 — with the conv bias as a fourth for a frozen block
        lib = _lib.load()
        B, Cc, H, W = plan.dims
        N, T, dev = H * W, B * H * W, x.device
        x = x.contiguous()
        d = GrapherBlock.from_buffer_copy(plan.tmpl)
        out = torch.empty((B, Cc, H, W), dtype=_F32, device=dev)
        out_tm = torch.empty((T, Cc), dtype=_F32, device=dev) if dual else None
        d.B, d.C, d.H, d.W = B, Cc, H, W
        d.x, d.out, d.out_tm = x.data_ptr(), out.data_ptr(), _ptr(out_tm)
        # the label block behind announced its graph: prepare its keys
        kk = knn_prep.KnnProblem.keys_for_label(B, Cc, N, label_knn) if (dual and fused.KNN_PREP) else None
        if kk is not None:
            ws = kk.workspace(lib, dev)                           # up front: the producer runs inside the call below
            d.keys_G, d.keys_L, d.keys_k, d.keys_d, d.keys_fused_mr, d.keys_flags = kk.G, kk.N, kk.k, kk.d, kk.fused_mr, kk.flags
            d.keys_ws, d.keys_ws_bytes = ws.data_ptr(), ws.numel()
        buf, _, _ = _forward(lib, plan, d, dev, N, N, relative_pos, False, False, None, "gkg_grapher_fwd")
        if kk is not None:
            kk.mark(out_tm)
        ctx.save_for_backward(buf, *params[::plan.stride])
        ctx.desc = d
        ctx.plan = plan
        if dual:
            ctx.set_materialize_grads(False)
            return out, out_tm
        return out

    @staticmethod
    def backward(ctx, dout, dtm=None):
        plan = ctx.plan
        B, Cc, H, W = plan.dims
        if dout is None and dtm is None:
            return (None,) * (5 + len(plan.params))
        buf, *weights = ctx.saved_tensors
        dev, d = buf.device, ctx.desc
        dx = torch.empty((B, Cc, H, W), dtype=_F32, device=dev)
        if dout is None:                                          # only the token-major companion was used downstream
            dout = torch.zeros((B, Cc, H, W), dtype=_F32, device=dev)
        dout_c = dout.contiguous()
        dtm_c = None if dtm is None else dtm.contiguous()
        d.dout, d.dout_tm, d.dx = dout_c.data_ptr(), _ptr(dtm_c), dx.data_ptr()
        return _backward(ctx, buf, weights, (dx, None, None, None, None), (dout_c, dtm_c), "gkg_grapher_bwd")


def _run_grapher(plan, mod, x, relative_pos, dual):
    res = _GrapherBlockFn.apply(x, plan, relative_pos, knn_prep.announced(mod), dual, *plan.params)
    out = res[0] if dual else res
    if dual:
        out._gkg_tm = (out._version, res[1])
    if fused.DUAL_LAYOUT:
        out._gkg_producer = weakref.ref(mod)
    return out


def grapher_forward(mod, x, relative_pos, groups, dual):
    """After grapher_ok(): the block through the driver (fused.grapher_forward; builds the plan the next calls go through)."""
    return _run_grapher(_plan_grapher(mod, x, relative_pos, groups), mod, x, relative_pos, dual)


def try_grapher(mod, x):
    """Grapher.forward's first question: a step this module has taken before (same shapes, same switches, same tensors behind the
    same names) goes straight to the driver -> the block's output; None: ask the long way (fused.fused_supported ...)."""
    plans = _PLANS.get(mod)
    if plans is None or not (ENABLED and x.is_cuda and x.dtype == _F32 and torch.is_grad_enabled()
                             and not torch.is_autocast_enabled()):
        return None
    plan = plans.get(("g", tuple(x.shape), mod.graph_conv.num_head, _switches()))
    if plan is None or not plan.fast or not x.is_contiguous() or not plan.valid():
        return None
    return _run_grapher(plan, mod, x, plan.rp, fused.DUAL_LAYOUT and mod.__dict__.get("_gkg_want_tm", False))


# ----------------------------------------------------------------------------------------------- GrapherLabel
class _LabelBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e2, ft, plan, keys_key, producer, *params):
        # params: (W, gamma, beta) of fc1, the grouped projection, fc2, FFN fc1 and FFN fc2 — + the conv bias for a frozen block
        lib = _lib.load()
        B, Cc, L, M, Cf = plan.dims
        T, dev = B * L, e2.device
        d = LabelBlock.from_buffer_copy(plan.tmpl)
        out = torch.empty((T, Cc), dtype=_F32, device=dev)
        d.B, d.C, d.L, d.M = B, Cc, L, M
        d.e, d.ft, d.out = e2.data_ptr(), ft.data_ptr(), out.data_ptr()
        buf, key, edge = _forward(lib, plan, d, dev, L, M, None, True, True, keys_key, "gkg_grapher_label_fwd")
        if fused.KNN_PREP:
            key.announce(producer, plan.groups, L)       # the Grapher in front prepares this graph's keys from its next call on
        ctx.save_for_backward(buf, e2, ft, *params[::plan.stride])
        ctx.desc = d
        ctx.plan = plan
        ctx.mark_non_differentiable(edge)
        ctx.set_materialize_grads(False)
        return out, edge

    @staticmethod
    def backward(ctx, dout, _gedge=None):
        plan = ctx.plan
        if dout is None:
            return (None,) * (5 + len(plan.params))
        B, Cc, L, M, Cf = plan.dims
        buf, e2, ft, *weights = ctx.saved_tensors
        dev, d = buf.device, ctx.desc
        de = torch.empty((B * L, Cc), dtype=_F32, device=dev)
        dft = torch.empty((B, M, Cc), dtype=_F32, device=dev)
        dout_c = dout.contiguous()
        d.dout, d.de, d.dft = dout_c.data_ptr(), de.data_ptr(), dft.data_ptr()
        return _backward(ctx, buf, weights, (de, dft, None, None, None), (e2, dout_c), "gkg_grapher_label_bwd")


def label_forward(mod, e2, ft, groups, keys_key, producer=None):
    """After label_ok(): the block through the driver (fused.grapher_label_forward; builds the plan the next calls go through)."""
    plan = _plan_label(mod, e2, ft, groups)
    return _LabelBlockFn.apply(e2, ft, plan, keys_key, producer, *plan.params)


def try_label(mod, e, features):
    """GrapherLabel.forward's first question (see try_grapher): -> (E', edge_index) or None."""
    plans = _PLANS.get(mod)
    if plans is None or not (ENABLED and e.is_cuda and e.dtype == _F32 and e.dim() == 3 and e.is_contiguous() and features.is_cuda
                             and features.dtype == _F32 and features.dim() == 4 and torch.is_grad_enabled()
                             and not torch.is_autocast_enabled()):
        return None
    B, L, Cc = e.shape
    if features.shape[0] != B or features.shape[1] != Cc or fused.is_channels_last(features):
        return None
    key = ("l", B * L, (B, features.shape[2] * features.shape[3], Cc), mod.graph_conv.num_head, _switches())
    plan = plans.get(key)
    if plan is None or not plan.valid():
        return None
    ft, keys_key, producer = fused._label_features(features, B, Cc)
    out, edge = _LabelBlockFn.apply(e.view(B * L, Cc), ft, plan, keys_key, producer, *plan.params)
    return out.view(B, L, Cc), edge
