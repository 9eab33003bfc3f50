"""Fused token-major execution of the Grapher / GrapherLabel blocks on the GPU.

Same math as the composable modules in ``graph.py`` / ``grapher.py`` (and therefore as the reference,
torch_vertex.py:278-403), restructured for MI355X:

* activations inside the block are token-major ``(B*N, C)``: every 1x1 projection is ONE large fp32 GEMM
  (vendor library, MFMA) instead of 32 per-image ones, and a graph neighbour is one contiguous row segment;
* everything between two GEMMs is a hand-written bandwidth kernel from ``libgkg_hip.so``
  (``csrc/gkg_dense.hip``): train-mode BN statistics (deterministic two-stage), BN-apply (+GELU) (+residual),
  the BN/GELU backward pair, layout changes fused into the first/last kernel of the block;
* the reference's interleave ``[x_0, m_0, x_1, m_1, ...]`` (torch_vertex.py:57-61) is never built: the grouped projection reads
  ONE operand buffer XM (T, 2C) whose conv-group columns are ordered [x chunk | m chunk] (include/gkg_hip.h "XM layout"); fc1's
  BN-apply writes x straight into its x chunks, the aggregation fills the m chunks, the permutation lives in the weight planes,
  and the backward's input-gradient GEMM writes dXM in the same layout for the scatter to read.

Autograd sees four custom Functions (layout, linear+BN+act, grouped linear+BN+act, max-relative) with
hand-written backward passes.  Used automatically by ``Grapher`` / ``GrapherLabel`` when supported
(``fused_supported``); everything else takes the composable path.  The handshake by which a BN-apply pass prepares the
tokens of the k-NN call behind it (round 6) lives in ``knn_prep.py``; here are its policy switches and its two kinds of call.
"""
from __future__ import annotations

import ctypes
import os
import weakref

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _lib, bn_passes, derived
from .ops import _ptr, _stream
from .parallel import grad_view

_F32 = torch.float32
ENABLED = True          # set False to force the composable (per-op) path, e.g. in A/B tests


def _env_list(name):
    return {t.strip() for t in os.environ.get(name, "").split(",") if t.strip()}


# ---- run-time switches (all of them; INTEGRATION.md has the table) ---------------------------------------------------
# GKG_GEMM_MATH — arithmetic of the fp32 projection GEMMs:
#   "x6" (default)  bf16 matrix cores with every fp32 operand split exactly into three bf16 terms, six cross products, fp32
#                   accumulation (csrc/gkg_gemm_x6.hip: error vs fp64 3-4x below an fp32 fma chain) for every forward, input-
#                   gradient and weight-gradient GEMM of the blocks (split-K forms for the label branch's short matrices, the
#                   weight gradients of a backward pass batched into one launch) — no vendor GEMM in the step;
#   "vendor"        vendor GEMM library + stand-alone BN passes everywhere (what autocast callers get anyway).
GEMM_MATH = os.environ.get("GKG_GEMM_MATH", "x6")
if GEMM_MATH not in ("x6", "vendor"):
    raise ValueError(f"GKG_GEMM_MATH={GEMM_MATH!r}: expected x6 | vendor")
# GKG_DETERMINISTIC=1 — run-to-run bit-identical backward: the neighbour-gradient scatter is order-independent by
# construction (exact fixed-point accumulation, gkg_mr_bwd_tm); the atomically accumulated x6 weight gradients and the
# fp64-atomic BN statistics give way to the library GEMM / the two-stage reductions (GKG_ENABLE=wgrad_det keeps the weight
# gradients on the x6 kernels instead, in their run-independent form).
DETERMINISTIC = os.environ.get("GKG_DETERMINISTIC", "0") != "0"
# GKG_ENABLE — comma-separated list of OPT-IN modes (off by default):
#   knn_bf16       under bf16 autocast the k-NN distance contraction runs on the bf16 matrix cores (GKG_KNN_BF16_CONTRACT:
#                  the reference computes this product in bf16 there too, and additionally rounds it to bf16).  Outside the
#                  bit-exact index contract (neighbour-set agreement 0.91-0.997 with the exact graph), hence
#                  opt-in since round 4: by default autocast callers get the SAME graphs as fp32 callers (north_star:
#                  "bit-exact neighbor indices"); bench.py --workload cfg3 / cfg5 prints both legs.
#   knn_f16        under CUDA autocast of either 16-bit dtype the contraction runs on the fp16 matrix cores instead
#                  (GKG_KNN_F16_CONTRACT: normalised tokens lie in [-1, 1], where fp16 keeps three more significand bits than
#                  bf16 at the same matrix-core rate — about eight times fewer changed neighbours; under fp16 autocast
#                  the reference itself contracts in fp16).  Outside the bit-exact index contract like knn_bf16, hence opt-in.
#                  With both switches on, knn_bf16 wins where it acts (bf16 autocast): bench.py flips KNN_BF16 for its second
#                  leg, so GKG_ENABLE=knn_f16 python bench.py --workload cfg3 times fp16 (first leg) and bf16 in one process.
#   lin_bf16       bf16 inference on the channels-last chain: the four dense projections of a Grapher + FFN pair (fc1, fc2,
#                  FFN.fc1, FFN.fc2) run on the library's own bf16 kernel with eval-mode BN, GELU, the fp32 residual and both
#                  output precisions in its epilogue (gkg_linear_bf16; linear_bf16.py) instead of the vendor GEMM (+ a stand-alone
#                  affine pass).  The BN scale stays fp32 (the weight is not folded), so fc1's rounding differs from the default
#                  path's.  Opt-in until its per-shape measurements decide the default (EXPERIMENTS.md).
#   lin_bf16_prep  with lin_bf16 only: a Grapher's fc1 launch also prepares its output as the k-NN's queries (normalised copies,
#                  |t|^2, prefilter planes: gkg_linear_bf16_knn_prep; linear_bf16.py) — the last workgroup of a row tile runs the
#                  preparation on the rows the tile completed, and the k-NN call behind it (GKG_KNN_X_PREPARED) launches no
#                  token preparation for the queries.  Same bits as lin_bf16 alone.  Not with knn_bf16 / knn_f16 or a patched knn_graph_tm.
#                  Taken only at the shapes where it measured at least as fast as the two launches (linear_bf16.prep_pays: the
#                  stage-1 shapes of cfg3 / cfg5); lin_bf16_prep_all takes it wherever the library accepts the shape (tests,
#                  measurements).
#   ffn_bf16       with lin_bf16 only: an FFN's two projections (fc1 + BN + GELU, fc2 + BN + residual) as ONE launch that keeps the
#                  (T, 4C) bf16 hidden matrix in LDS instead of writing it and reading it back (gkg_ffn_bf16; linear_bf16.py).
#                  Same bits as lin_bf16 alone.  C <= 192 (the stages with the most rows); wider FFNs, an active DropPath, NCHW
#                  input and the label branch keep the two launches.  Opt-in: per-shape measurements in EXPERIMENTS.md.
#   mr_fc2_bf16    with lin_bf16 only (and mr_gemm not disabled): the second half of a Grapher on the channels-last chain — aggregation +
#                  grouped projection + BN + GELU, then fc2 + BN + residual — as ONE launch that keeps the (T, 2C) bf16 matrix
#                  between the two projections in LDS instead of writing it and reading it back (gkg_mr_fc2_bf16; linear_bf16.py).
#                  Same bits as lin_bf16 alone.  C <= 192 (the stages with the most rows); wider Graphers, an active DropPath, NCHW
#                  input and the label branch keep the two launches.  Taken only at the shapes where it measured at least as fast
#                  as the two launches (linear_bf16.mr_fc2_pays); mr_fc2_bf16_all takes it wherever the library accepts the shape
#                  (tests, measurements).
#   train_bf16     training under bf16 autocast: the three products of a dense projection of a Grapher / FFN block (_LinearBNAct under
#                  autocast: Y = x W^T, dx = dY W (+ the skip gradient), dW = dY^T x) run on the library's own bf16 kernels — bf16
#                  operands rounded from the fp32 tensors on their way into LDS, fp32 accumulation (gkg_linear_bf16_f32a,
#                  gkg_linear_wgrad_bf16; linear_bf16.py) — instead of the autocast vendor GEMM with its casts, the fp32 vendor GEMM
#                  and the six-product x6 weight gradient.  bf16 autocast with gradients only; not under GKG_DETERMINISTIC (the
#                  weight gradient adds its row slabs atomically); the grouped projection, fp16 autocast and the BN passes keep
#                  their paths.  Opt-in: per-layer measurements in EXPERIMENTS.md.
#   train_f16      training under fp16 autocast (the reference's recipe: fp16 AMP with a dynamic loss scale): the forward Y = x W^T and
#                  the input gradient dx = dY W (+ the skip gradient) of the same layers run on the fp16 form of the own kernel —
#                  IEEE fp16 operands rounded from the fp32 tensors on their way into LDS (subnormals kept), fp32 accumulation
#                  (gkg_linear_f16_f32a; linear_bf16.py) — instead of the autocast vendor GEMM with its casts and the fp32 vendor
#                  GEMM.  The weight gradient stays where it is (_wgrad), so the switch adds nothing atomically and also holds
#                  under GKG_DETERMINISTIC.  fp16 autocast with gradients only; bf16 autocast, fp32, fp16 inference, the grouped
#                  projection and the BN passes keep their paths.  May be on together with train_bf16: each acts under its own
#                  autocast dtype.  Opt-in: per-layer measurements in EXPERIMENTS.md.
#   train_grouped  an add-on to train_bf16 / train_f16 (alone it does nothing): the GROUPED projection between a Grapher's dense
#                  layers (BasicConv's Conv2d 1x1, groups = 4, behind the max-relative aggregation) takes its forward Y_q = XM_q W_q^T
#                  and its input gradient dXM_q = dY_q W_q from ONE launch each of the own kernel's grouped form
#                  (gkg_linear_bf16_f32a_grouped / gkg_linear_f16_f32a_grouped; linear_bf16.py) under the kind's autocast dtype —
#                  instead of the autocast vendor bmm on a gathered 16-bit copy of the strided operand view with its widening pass,
#                  and the fp32 vendor bmm with its re-layout copy.  Nothing atomic: holds under GKG_DETERMINISTIC for both kinds.
#                  The grouped weight gradient, the BN passes, the block driver and XM_DIRECT keep their paths.  With it off every
#                  launch of every other switch combination is what it was.  Opt-in: per-layer measurements in EXPERIMENTS.md.
#   wgrad_det     with GKG_DETERMINISTIC=1 and GKG_GEMM_MATH=x6 only: the projections' weight gradients stay on the library's x6
#                  kernels in their run-independent form (gkg_linear_wgrad_x6_det / _batch_det: the row slabs' partial tiles go to
#                  a workspace and are added in slab order; no atomics, no cleared slot) instead of the vendor batched GEMM + sum —
#                  the XM operand view with its column permutation included, and batched into one launch per backward pass like
#                  the default path.  Bit-identical from run to run, but other bits than the vendor path's.  Without
#                  GKG_DETERMINISTIC it does nothing.  Opt-in: measurements in EXPERIMENTS.md.
# GKG_DISABLE — comma-separated list of optimisations to switch off (A/B measurements).  Round 6 cut the list to the eight
# structural ones (the per-kernel switches of rounds 2-5 are gone with the alternatives they selected):
#   knn_mr         k-NN + aggregation as one kernel (row g2)          knn_compact   u16 neighbour lists between two launches
#   block_driver   a block's forward / backward as ONE library call     wgrad_batch   one weight-gradient launch per backward
#   dual_layout    a Grapher's output in both layouts for a label block
#   mr_gemm        bf16 inference: aggregation as the grouped projection's operand producer (row g1)
#   channels_last  blocks take / return channels-last tensors as views of their token-major matrices
#   fold_epilogue  bf16 inference: eval-mode BN folded into the weights, bias (+ GELU) in the library GEMM's epilogue
#   bwd_fuse       backward: BN statistics taken by the kernel that produces the gradient (re-layout pass, aggregation scatter),
#                  a Grapher's dx stored channel-major by its input-gradient GEMM (BWD_FUSE below)
#   dgrad_stats    backward: BN statistics taken by the input-gradient GEMM that writes the layer's upstream gradient, at every
#                  size (DGRAD_STATS below; bwd_fuse off switches it off too)
#   x6_walk        projection launches of two rounds of resident workgroups as one round of workgroups that each walk a static
#                  list of tiles (X6_WALK below; csrc/gkg_gemm_x6_tile.h)
_DISABLED = _env_list("GKG_DISABLE")
_ENABLED = _env_list("GKG_ENABLE")
KNN_BF16 = "knn_bf16" in _ENABLED
KNN_F16 = "knn_f16" in _ENABLED            # likewise a module constant (tests and bench legs flip them)
LIN_BF16 = "lin_bf16" in _ENABLED          # a module constant the tests flip (like MR_GEMM)
# likewise (False | True: the measured shapes | "all": every supported shape); acts only together with LIN_BF16
LIN_BF16_PREP = "all" if "lin_bf16_prep_all" in _ENABLED else ("lin_bf16_prep" in _ENABLED)
FFN_BF16 = "ffn_bf16" in _ENABLED          # likewise; acts only together with LIN_BF16
# likewise (False | True: the measured shapes | "all": every supported shape); acts only together with LIN_BF16 and MR_GEMM
MR_FC2_BF16 = "all" if "mr_fc2_bf16_all" in _ENABLED else ("mr_fc2_bf16" in _ENABLED)
TRAIN_BF16 = "train_bf16" in _ENABLED      # likewise a module constant the tests flip
TRAIN_F16 = "train_f16" in _ENABLED        # likewise
TRAIN_GROUPED = "train_grouped" in _ENABLED    # likewise; acts only together with TRAIN_BF16 / TRAIN_F16, each under its own autocast dtype
WGRAD_DET = "wgrad_det" in _ENABLED        # likewise; acts only together with DETERMINISTIC and GEMM_MATH == "x6"


from .planes import (_WeightPlanes, _PLANES, _planes, refresh_weight_planes, param_version,      # noqa: E402,F401  (x6 weight
                     mark_parameters_updated)                                                 # planes + staleness: planes.py)


def _x6(x, weight, bn, nb=1, kind="fwd", group=...) -> bool:
    """This projection GEMM (kind "fwd": y = x W^T, "dgrad": dx = dy W) runs on the x6 kernels.  Eligible: fp32 operands
    outside autocast, batch statistics local to the rank or exchanged in fp64 (_sync_x6_ok), 16-byte aligned rows, the C entry
    points' size limits (_x6_rule).  ``group``: bn's statistics group when the caller has asked already (_sync_group)."""
    if GEMM_MATH != "x6":
        return False
    if group is ...:
        group = _sync_group(bn)
    if not (x.dtype == _F32 and weight.dtype == _F32 and not torch.is_autocast_enabled() and _sync_x6_ok(group)
            and x.shape[-1] % 4 == 0 and weight.shape[0] % 4 == 0):
        return False
    return _x6_rule(x.shape[-2], x.shape[-1], weight.shape[0] // nb, nb, kind)


def _x6_rule(R, cin, cout, nb, kind) -> bool:
    """The shape part of _x6 (operand dtypes / autocast / SyncBN already checked by the caller): the C entry points' own limits
    (gkg_linear_bn_fwd_x6 / gkg_linear_dgrad_x6 return GKG_ERR_UNSUPPORTED / _SHAPE beyond them) — per-group widths multiples of
    4, at most 64 groups, operands below 4 GiB per batch, the statistics scratch.  (Rounds 2-4 applied a per-shape rule against
    the vendor library here; it went away with the split-K forms, the residual epilogue and the batched weight gradients.)"""
    if GEMM_MATH != "x6":
        return False
    return not (cout % 4 or nb > 64 or R * max(cin, cout) * 4 > 0xffffffff
                or nb * 2 * cout > _lib.load().gkg_linear_stats_doubles())


def _mr_bwd_flags() -> int:
    return _lib.MR_DETERMINISTIC if DETERMINISTIC else 0


def _x6_wgrad_ok(dY, x, nb=1) -> bool:
    """The streaming x6 weight-gradient kernel (gkg_linear_wgrad_x6: both operands split in registers, each wave copies its
    own rows through a private LDS ring by DMA; row slabs placed per XCD; fp32 atomics into the zeroed dW, i.e. a run-dependent
    summation order — GKG_DETERMINISTIC=1 keeps the library GEMM)."""
    if GEMM_MATH != "x6" or dY.dtype != _F32 or x.dtype != _F32 or DETERMINISTIC:
        return False
    return max(dY.stride(-2), x.stride(-2)) * 4 * 16 <= 0x7fffffff and nb <= 64     # gkg_linear_wgrad_x6's row-pitch / batch limits


def _x6_wgrad_det_ok(dY, x, nb=1) -> bool:
    """The same kernels in their run-independent form (gkg_linear_wgrad_x6_det: every slab's partial tile stored to a workspace,
    the slabs added in row order by a second small launch) — what GKG_DETERMINISTIC=1 runs with GKG_ENABLE=wgrad_det."""
    if GEMM_MATH != "x6" or dY.dtype != _F32 or x.dtype != _F32 or not (DETERMINISTIC and WGRAD_DET):
        return False
    return max(dY.stride(-2), x.stride(-2)) * 4 * 16 <= 0x7fffffff and nb <= 64     # gkg_linear_wgrad_x6's row-pitch / batch limits


def _wgrad_det_call(dY, ldg, g_bs, x, ldx, x_bs, out, R, cin, cout, nb, kperm, what):
    """gkg_linear_wgrad_x6_det with the library's slab rule, the device's workspace (wgrad_queue.det_workspace) and the slot as
    it is: the call overwrites every element."""
    lib = _lib.load()
    ws = _det_workspace(x.device, lib.gkg_linear_wgrad_x6_det_workspace_bytes(R, cin, cout, nb, ldg, ldx, 0))
    _lib.check(lib.gkg_linear_wgrad_x6_det(_ptr(dY), ldg, g_bs, _ptr(x), ldx, x_bs, _ptr(out), R, cin, cout, nb, kperm, 0, _ptr(ws),
                                           ws.numel(), _stream()), what)
    return out


# ---- batched weight gradients (round 5) ---------------------------------------------------------------------------------
# wgrad_queue.py owns the queue and its protocol; here is the policy, what goes into it.  Queued only when the gradient has a slot
# in a GradBucket (the kernel writes there; autograd adopts the returned view as ``p.grad``; GradBucket flushes the queue before
# it reads a gradient) — without a bucket autograd consumes the returned tensor at once, so the node launches its own dW, as
# before.  GKG_DISABLE=wgrad_batch: every weight gradient in its own launch.
WGRAD_BATCH = "wgrad_batch" not in _DISABLED
WGRAD_UNITS = 0          # rows per workgroup of the batched launch / 128 (0: the library's default, 20)

from . import parallel as _parallel      # noqa: E402
from . import planes as _planes_mod      # noqa: E402
from .wgrad_queue import QUEUE as _WQ, det_workspace as _det_workspace    # noqa: E402
_parallel._ZERO_DEFER[:] = [_planes_mod.defer_zero, _planes_mod.flush_deferred_zero]


def flush_wgrads():
    """Launch every queued weight gradient (no-op when the queue is empty)."""
    _WQ.flush()


def _wgrad_queue(device):
    """The queue to defer a weight gradient into right now (opened for the running backward pass on the current stream), or None:
    batching switched off, or no backward pass that would flush it.  Under GKG_DETERMINISTIC it opens only for the run-independent
    launch (WGRAD_DET: gkg_linear_wgrad_x6_batch_det)."""
    if not (WGRAD_BATCH and (WGRAD_DET or not DETERMINISTIC) and GEMM_MATH == "x6"):
        return None
    task = _WQ.task_id()
    return _WQ.open(task, device, WGRAD_UNITS, det=DETERMINISTIC) if task >= 0 else None


def _wgrad_defer(dY, x, out, R, cin, cout, nb, ldg, g_bs, ldx, x_bs, kperm=0) -> bool:
    """Queue dW = dY^T x for the batched launch.  True: queued (``out`` will hold the gradient when the backward pass ends)."""
    if not (out is not None and getattr(out, "_gkg_slot", False) and dY.dtype == _F32 and x.dtype == _F32
            and R % 128 == 0 and cin % 4 == 0 and cout % 4 == 0 and ldg % 4 == 0 and ldx % 4 == 0 and g_bs % 4 == 0 and x_bs % 4 == 0
            and dY.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and R * max(ldg, ldx) * 4 < 0xffffffff and nb <= 64):
        return False
    # a problem that fills the chip on its own (GKGNet-576's stage-1 / stage-2 layers: thousands of 128-row units) is launched from
    # the node: that costs nothing and frees its operands.  This is a SEPARATE, coarser rule than the library's: inside a batch the
    # library keeps a problem's stand-alone slabs when tiles * stand-alone slab count >= 512 (csrc/gkg_x6_plan.h x6_wgrad_fills_chip,
    # over the tile shape x6_wgrad_plan picks); the test below only decides which problems are queued at all, and the two are not
    # the same predicate.
    tiles = nb * ((cout + 63) // 64) * ((cin + 63) // 64)
    if tiles * min(R // 128, 64) >= 2048 and R >= 32768:
        return False
    q = _wgrad_queue(dY.device)
    if q is None:
        return False
    if not q.det and not getattr(out, "_gkg_zero", False):       # (the run-independent launch overwrites the slot)
        out.zero_()
    q.push((_lib.WgradProblem(dY.data_ptr(), x.data_ptr(), out.data_ptr(), g_bs, x_bs, ldg, ldx, R, cin, cout, nb, kperm),), (out,),
           (dY, x))
    return True


def _wgrad_defer_block(problems, n, outs, keep, device) -> bool:
    """The block driver's weight-gradient problems (prebuilt GkgWgradProblem array, dW slots already zero): all of them into the
    backward pass's batched launch, or none (False: the caller launches them now)."""
    if not (all(getattr(o, "_gkg_slot", False) for o in outs) and all(problems[i].R % 128 == 0 for i in range(n))):
        return False
    q = _wgrad_queue(device)
    if q is None:
        return False
    q.push([_lib.WgradProblem.from_buffer_copy(problems[i]) for i in range(n)], outs, keep)
    return True


def _wgrad(dY: torch.Tensor, x: torch.Tensor, out=None) -> torch.Tensor:
    """dW (Cout, Cin) = dY^T (Cout x R) @ x (R x Cin).  The output is tiny and the contraction long (R = B*N),
    so a single GEMM leaves most CUs idle; split R into S slabs with a batched GEMM and add the S partials.
    ``out``: the parameter's slot in the gradient bucket (written in place, see parallel.grad_view)."""
    R = x.shape[0]
    if out is not None and out.dtype != dY.dtype:
        out = None
    if (dY.stride(1) == 1 and x.stride(1) == 1
            and _wgrad_defer(dY, x, out, R, x.shape[1], dY.shape[1], 1, dY.stride(0), 0, x.stride(0), 0)):
        return out
    if _x6_wgrad_ok(dY, x) and dY.stride(1) == 1 and x.stride(1) == 1 and dY.stride(0) % 4 == 0 and x.stride(0) % 4 == 0:
        cout, cin = dY.shape[1], x.shape[1]
        if out is None:
            out = torch.zeros((cout, cin), dtype=_F32, device=x.device)
        elif not getattr(out, "_gkg_zero", False):          # a bucket slot cleared by GradBucket.release(prezero=True) is clean
            out.zero_()
        _lib.check(_lib.load().gkg_linear_wgrad_x6(_ptr(dY), dY.stride(0), 0, _ptr(x), x.stride(0), 0, _ptr(out), R, cin, cout,
                                                   1, 0, _stream()), "gkg_linear_wgrad_x6")
        return out
    if _x6_wgrad_det_ok(dY, x) and dY.stride(1) == 1 and x.stride(1) == 1 and dY.stride(0) % 4 == 0 and x.stride(0) % 4 == 0:
        cout, cin = dY.shape[1], x.shape[1]
        if out is None:
            out = torch.empty((cout, cin), dtype=_F32, device=x.device)
        return _wgrad_det_call(dY, dY.stride(0), 0, x, x.stride(0), 0, out, R, cin, cout, 1, 0, "gkg_linear_wgrad_x6_det")
    if R >= 4096:                # short contractions (the label branch): the partial-sum kernel costs more than it saves
        for S in (8, 6, 4, 3, 2):
            if R % S == 0 and R // S >= 1024:
                part = torch.bmm(dY.view(S, R // S, -1).transpose(1, 2), x.view(S, R // S, -1))
                return part.sum(0) if out is None else torch.sum(part, 0, out=out)
    return torch.mm(dY.t(), x) if out is None else torch.mm(dY.t(), x, out=out)


def _kperm_weight(Wg: torch.Tensor) -> torch.Tensor:
    """(nb, co, ci) weight with its input columns as [even | odd]: the order an XM operand buffer presents them in (the x
    chunk, then the m chunk) — for the GEMM paths that read the weight tensor itself rather than its x6 planes (and, through
    derived.glin_planes, for the fragment arrays of the own grouped 16-bit products)."""
    return derived.kperm_weight(Wg)


def _kperm_grad_back(dWp: torch.Tensor, out=None) -> torch.Tensor:
    """Inverse of _kperm_weight on a gradient: columns [x chunk | m chunk] -> the reference's interleave."""
    nb, co, ci = dWp.shape
    dW = dWp.view(nb, co, 2, ci // 2).permute(0, 1, 3, 2).reshape(nb, co, ci)
    if out is None:
        return dW
    out.copy_(dW)
    return out


def _wgrad_grouped(dY: torch.Tensor, U: torch.Tensor, out=None, kperm=0) -> torch.Tensor:
    """Grouped projection: dW[q] (co, ci) = dY[q]^T @ U[q] for the nb groups; long contractions are split like
    ``_wgrad`` (nb*S batched GEMMs + one partial sum).  ``U`` (nb, R, ci) may be a strided view (the XM operand buffer:
    strides (ci, 2C, 1)); ``kperm``: its columns are [x chunk | m chunk] and dW is returned in the reference's interleaved
    column order (the x6 kernels permute where they add their tiles to dW)."""
    nb, R, co = dY.shape
    ci = U.shape[2]
    S = 4
    if out is not None and (out.dtype != dY.dtype or not out.is_contiguous()):
        out = None
    if (dY.stride(2) == 1 and U.stride(2) == 1
            and _wgrad_defer(dY, U, out, R, ci, co, nb, dY.stride(1), dY.stride(0), U.stride(1), U.stride(0), kperm)):
        return out
    if (_x6_wgrad_ok(dY, U, nb) and dY.stride(2) == 1 and U.stride(2) == 1
            and all(t.stride(d) % 4 == 0 for t in (dY, U) for d in (0, 1))):
        if out is None:
            out = torch.zeros((nb, co, ci), dtype=_F32, device=U.device)
        elif not getattr(out, "_gkg_zero", False):
            out.zero_()
        _lib.check(_lib.load().gkg_linear_wgrad_x6(_ptr(dY), dY.stride(1), dY.stride(0), _ptr(U), U.stride(1), U.stride(0), _ptr(out),
                                                   R, ci, co, nb, kperm, _stream()), "gkg_linear_wgrad_x6 (grouped)")
        return out
    if (_x6_wgrad_det_ok(dY, U, nb) and dY.stride(2) == 1 and U.stride(2) == 1
            and all(t.stride(d) % 4 == 0 for t in (dY, U) for d in (0, 1))):
        if out is None:
            out = torch.empty((nb, co, ci), dtype=_F32, device=U.device)
        return _wgrad_det_call(dY, dY.stride(1), dY.stride(0), U, U.stride(1), U.stride(0), out, R, ci, co, nb, kperm,
                               "gkg_linear_wgrad_x6_det (grouped)")
    if kperm:
        return _kperm_grad_back(_wgrad_grouped(dY, U.contiguous() if R >= 4096 else U, None, 0), out)
    if R >= 4096 and R % S == 0 and U.is_contiguous():
        part = torch.bmm(dY.reshape(nb * S, R // S, co).transpose(1, 2), U.reshape(nb * S, R // S, ci))
        return part.view(nb, S, co, ci).sum(1) if out is None else torch.sum(part.view(nb, S, co, ci), 1, out=out)
    return torch.bmm(dY.transpose(1, 2), U) if out is None else torch.bmm(dY.transpose(1, 2), U, out=out)


_STATS = {}


def _stats_scratch(device) -> torch.Tensor:
    """fp64 column-sum scratch of the projection kernels' BN-statistics epilogue: zero on entry, re-zeroed by the
    finalize kernel of every call, so ONE buffer per device serves all layers (stream-ordered)."""
    key = (device.type, device.index)
    t = _STATS.get(key)
    if t is None:
        t = torch.zeros(_lib.load().gkg_linear_stats_doubles(), dtype=torch.float64, device=device)
        _STATS[key] = t
    return t


_SK = {}


def _sk_ws(device) -> torch.Tensor:
    """Split-K workspace of the x6 projection kernels (tile counters + partial tiles; include/gkg_hip.h): one per device,
    counters zero between launches, stream-ordered reuse."""
    key = (device.type, device.index)
    t = _SK.get(key)
    if t is None:
        t = torch.zeros(_lib.load().gkg_x6_splitk_workspace_bytes(), dtype=torch.uint8, device=device)
        _SK[key] = t
    return t


def _dgrad_x6(lib, dY, ldg, g_bs, pd, dx, R, cin, cout, nb, residual=None, ldx=0, x_bs=0):
    """dx = dY W (+ residual: the skip connection's gradient, added in the epilogue) on the x6 kernel.  ``ldx`` / ``x_bs``: row
    pitch / batch stride of dx (0: contiguous (nb, R, cin)) — the grouped projection writes dXM (R, 2C) with (2C, C/2)."""
    ws = _sk_ws(dY.device)
    _lib.check(lib.gkg_linear_dgrad_x6_sk(_ptr(dY), ldg, g_bs, _ptr(pd), _ptr(dx), R, cin, cout, nb, _ptr(residual), _ptr(ws),
                                          ws.numel(), ldx, x_bs, _x6_flags(), _stream()), "gkg_linear_dgrad_x6")


def _grad_outs(gparams, wshape, nch, dev):
    """Output tensors for (dW, dgamma, dbeta): the parameters' slots in the gradient bucket when they have one and the
    step is not accumulating (parallel.grad_view), else fresh tensors.  ``wshape`` None: a BN without a projection, no dW."""
    w = g = b = None
    if gparams is not None:
        wp, gp, bp = gparams
        w = grad_view(wp, wshape) if (wshape is not None and wp.dtype == _F32) else None
        g = grad_view(gp, (nch,)) if gp.dtype == _F32 else None
        b = grad_view(bp, (nch,)) if bp.dtype == _F32 else None
    if w is None and wshape is not None:
        w = torch.empty(wshape, dtype=_F32, device=dev)
    if g is None:
        g = torch.empty(nch, dtype=_F32, device=dev)
    if b is None:
        b = torch.empty(nch, dtype=_F32, device=dev)
    return w, g, b


def _project_bn(lib, x, planes, geom, mode=0, bn_args=(None,) * 10 + (0.0, 0.0), sums=None):
    """Y = x W^T on gkg_linear_bn_fwd_x6_sk.  ``geom`` = (R, cin, cout, nb); ``x``: a contiguous (R, cin) matrix or, nb > 1, a
    (nb, R, cin) tensor read through its strides (the XM operand buffer's groups); ``planes``: the weight's forward bf16 planes.
    ``mode`` 0: the product alone; 1: BN statistics in the epilogue + the finalize kernel (``bn_args``: gamma .. eps of the entry
    point, ``sums``: _stats_scratch); 2: the fp64 column sums only, into ``sums`` (a scratch-pair buffer: bn_passes.apply_from_sums
    reads them)."""
    R, cin, cout, nb = geom
    xld, xbs = (x.stride(1), x.stride(0)) if nb > 1 else (cin, R * cin)
    Y = torch.empty((nb, R, cout) if nb > 1 else (R, cout), dtype=_F32, device=x.device)
    ws = _sk_ws(x.device)
    _lib.check(lib.gkg_linear_bn_fwd_x6_sk(_ptr(x), xld, xbs, _ptr(planes), _ptr(Y), R, cin, cout, nb, mode, *bn_args, _ptr(sums),
                                           _ptr(ws), ws.numel(), _x6_flags(), _stream()),
               "gkg_linear_bn_fwd_x6 (statistics only)" if mode == 2 else "gkg_linear_bn_fwd")
    return Y


def _linear_fwd_own(lib, x, planes, geom, bias, bn):
    """Y, a, c, mean, invstd of BN(x W^T) through gkg_linear_bn_fwd_x6 (statistics in the GEMM epilogue + finalize kernel); x,
    planes and geom as _project_bn takes them."""
    n = geom[2] * geom[3]
    if not bn_passes.batch_stats(bn):
        return (_project_bn(lib, x, planes, geom),) + bn_passes.eval_ac(lib, bn, bias, n) + (None, None)
    a, c, mean, invstd = (torch.empty(n, dtype=_F32, device=x.device) for _ in range(4))
    Y = _project_bn(lib, x, planes, geom, 1, (_ptr(bn.weight), _ptr(bn.bias), _ptr(bias), *bn_passes.running_stats(bn), _ptr(a),
                                              _ptr(c), _ptr(mean), _ptr(invstd), float(bn.momentum), float(bn.eps)),
                    _stats_scratch(x.device))
    return Y, a, c, mean, invstd


def lowp_inference() -> bool:
    """bf16 autocast with gradients off: intermediates that only feed a projection GEMM (the block's token-major
    input, the aggregated [x, m] operand, FFN hidden activations) are written as bf16 by the producing kernel, and the
    GEMMs return fp32 directly (``out_dtype``) — no stand-alone cast kernels, half the bytes on those tensors."""
    return (not torch.is_grad_enabled() and torch.is_autocast_enabled()
            and torch.get_autocast_dtype("cuda") == torch.bfloat16)


FOLD_EPILOGUE = "fold_epilogue" not in _DISABLED


def _mm_t(x, W, W16=None):
    """x (R, cin) @ W (cout, cin)^T -> fp32 (R, cout).  bf16 ``x``: bf16 operands, fp32 accumulate AND fp32 result."""
    if x.dtype == torch.bfloat16:
        Wb = W.to(torch.bfloat16) if W16 is None else W16.view(W.shape)
        return torch.mm(x, Wb.t(), out_dtype=_F32)
    Y = torch.mm(x, W.t())               # under autocast: bf16 operands, fp32 accumulate
    return Y if Y.dtype == _F32 else Y.float()


from .linear_bf16 import (lin_bf16_ok, linear_bf16_eval,      # noqa: E402,F401  (GKG_ENABLE=lin_bf16: linear_bf16.py)
                          lin_bf16_prep_ok, linear_bf16_knn_prep_eval)
from .linear_bf16 import ffn_bf16_ok, ffn_bf16_eval      # noqa: E402,F401  (GKG_ENABLE=lin_bf16,ffn_bf16)
from .linear_bf16 import mr_fc2_bf16_ok, mr_fc2_bf16_eval      # noqa: E402,F401  (GKG_ENABLE=lin_bf16,mr_fc2_bf16)
from .linear_bf16 import (BF16, F16, train16_ok, train16_fwd,      # noqa: E402,F401  (GKG_ENABLE=train_bf16 / train_f16)
                          train16_dgrad, linear_bf16_wgrad)
from .linear_bf16 import (train16_grouped_ok, train16_grouped_fwd,      # noqa: E402,F401  (GKG_ENABLE=train_grouped beside them)
                          train16_grouped_dgrad)
from .layout import _tm_dtype, _TokenMajorToCL, _ToTokenMajor, _BlockEntry, _AvgPoolTM      # noqa: E402  (layout Functions: layout.py)


# ----------------------------------------------------------------------------------------------- layout
# A block whose input arrives channels-last — logical (B, C, H, W), memory (B, H, W, C): exactly the token-major matrix
# the block computes on — takes it as a VIEW and returns a channels-last tensor as well (same shape and values as the
# reference's output, different strides), so a chain of blocks never transposes: it saves nchw_to_tm + the transposing
# half of tm_affine_to_nchw per block and direction (12 % of the cfg3 forward, 6 % of the cfg4 step).  NCHW-contiguous
# inputs keep the NCHW-in / NCHW-out behaviour; the GKGNet backbone converts once after the stem and each downsample.
CHANNELS_LAST = "channels_last" not in _DISABLED


def is_channels_last(x) -> bool:
    return (CHANNELS_LAST and x.dim() == 4 and x.dtype == _F32 and x.shape[1] > 1 and x.shape[2] * x.shape[3] > 1
            and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last))



def _cl_out(out_tm, B, H, W):
    """Token-major block output -> channels-last tensor; a bf16 copy emitted by the last kernel rides along as an attribute
    (keyed on the tensor's version) for the next block's entry."""
    res = _TokenMajorToCL.apply(out_tm, B, H, W)
    o16 = getattr(out_tm, "_gkg_bf16_tm", None)
    if o16 is not None:
        res._gkg_bf16 = (res._version, o16)
    return res


def _block_entry(x, lp):
    """-> (GEMM operand (T, C), residual, channels_last?).  Channels-last input: both are views of x (bf16 inference: the
    operand is a cast copy); NCHW input: the layout kernel (_BlockEntry)."""
    if is_channels_last(x):
        B, C, H, W = x.shape
        xt = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
        if lp:
            # the producing block may have left the bf16 rounding of this very tensor (see _cl_out): no cast pass
            ent = getattr(x, "_gkg_bf16", None)
            x16 = ent[1] if ent is not None and ent[0] == x._version and ent[1].shape == xt.shape else xt.to(torch.bfloat16)
            return x16, xt, True
        return xt, xt, True
    xt, xr = _BlockEntry.apply(x.float().contiguous(), lp)
    return xt, xr, False



def to_token_major(x):
    return _ToTokenMajor.apply(x)



# ----------------------------------------------------------------------------------------------- BN: the policy
# Which launch sequence a BN layer's forward and backward take is decided here — the switches above and below, and the predicates
# _sync_group, _sync_x6_ok, _derive_ok, _bwd_fuse_ok, _bn_link, _bn_scale_in_kernel; the sequences themselves, every gkg_bn_* call
# and the record they read a layer from are bn_passes.py's, which gets the answers as arguments (``group``, ``atomic``).
def _sync_group(bn):
    """The process group this BN exchanges its batch statistics over (SyncBatchNorm in training under an
    initialised multi-rank group: the reference's DDP semantics), or None for local statistics."""
    if not (isinstance(bn, torch.nn.SyncBatchNorm) and bn.training and dist.is_available() and dist.is_initialized()):
        return None
    group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    return group if dist.get_world_size(group) > 1 else None


def _sync_x6_ok(group) -> bool:
    """Whether a layer with this statistics group (None: rank-local) may take the x6 projection kernels and the two-launch fp64
    BN passes.  Across ranks the fp64 column sums themselves are all-reduced (gkg_bn_apply_train_sync / gkg_bn_bwd_apply_sync);
    GKG_DETERMINISTIC keeps such a layer on the two-stage fp32 exchange (the fp64 atomics are run-dependent in their last bits)."""
    return group is None or (GEMM_MATH == "x6" and not DETERMINISTIC)


from .bn_scratch import _BnLink, _BnScratch      # noqa: E402  (the layer record + fp64 column-sum scratch of the two-launch BN passes)


def _project_apply(lib, x, planes, geom, bias, bn, group, dest, out_tm=None, prep=None):
    """Projection (statistics in its epilogue: _project_bn mode 2) -> BN-apply straight from the fp64 sums
    (bn_passes.apply_from_sums, which takes ``group`` .. ``prep``): two launches in one scope of the scratch pair, no finalize
    kernel -> (Y, a, c, mean, invstd, sync).  With a statistics group the row count rides in the double behind the sums."""
    R, _, cout, nb = geom
    with _BnScratch.of(x.device).scoped(lib, 2 * nb * cout + (group is not None)) as sums:
        Y = _project_bn(lib, x, planes, geom, 2, sums=sums[0])
        return (Y,) + bn_passes.apply_from_sums(lib, Y, sums, bn, bias, group, (R, cout, nb), dest, out_tm, prep)


def _derive_ok(bn, nb, cout, code, want16, group=...) -> bool:
    """Train-mode statistics (local to the rank, or exchanged as fp64 sums: _sync_x6_ok), fp32 output: the BN-apply pass
    derives its coefficients from the projection kernel's sums (no finalize launch).  ``group``: as in _x6."""
    if group is ...:
        group = _sync_group(bn)
    return (bn_passes.batch_stats(bn) and _sync_x6_ok(group)
            and code == _lib.F32 and not want16 and _BnScratch.fits(2 * nb * cout + (group is not None)))


# BN backward statistics in the epilogue of the NEXT projection's input-gradient GEMM (round 4, csrc/gkg_gemm_x6.hip X6_BNBWD).
# In h = act(BN(Y)) -> out = h W^T the gradient dh that the second layer's dgrad produces is the first layer's upstream
# gradient: the producer layer hangs a _BnLink on the tensor it returns; a consumer whose dgrad runs on the x6 kernel finds
# it on its input, lets the GEMM's epilogue accumulate  sum dz, sum dz yhat  (one extra read of Y, no pass over dh) and
# leaves the scratch buffers on the link; the producer's backward then runs the apply pass only.  MEASURED neutral (round 4,
# same-box A/B: cfg4 train step 90.0 / 90.4 ms with, 90.1 / 90.3 without; stage3 3.17-3.18 either way; cfg2 0.919 vs 0.915):
# the 16 y rows per lane, the GELU' recompute and the reduction sit on the tail of a workgroup that lives 10-15 us, which
# costs the GEMM what the removed pass (near the HBM roofline on its own) saved.  A later same-box A/B of the cfg4 step
# (alternating runs) measured 85.16 / 85.18 ms without and 84.70 / 84.67 ms with: on from 32 768 rows (below).
BN_EPILOGUE = True
# rows from which the link is attached: where the saved pass over the gradient is memory time (GKGNet-576's stages: cfg4 85.17 ->
# 84.69 ms on one box) rather than a launch among ~85 short ones (neutral at the cfg2 shapes, 10 368 rows).  The tests set
# BN_EPILOGUE_MIN_ROWS = 0 to attach it at every size.
BN_EPILOGUE_MIN_ROWS = 32768


# Backward passes folded into their producers (round 8).  Where the upstream gradient g of a train-mode BN layer (no activation)
# is written by a streaming kernel that holds every value in registers, that kernel also reads Y and takes  sum g, sum g yhat
# — gkg_nchw_to_tm_add_bnstats for a block's last layer (the NCHW -> token-major re-layout of the block output's gradient),
# gkg_mr_bwd_tm_bnstats for a Grapher's / GrapherLabel's fc1 (the aggregation's scatter) — and the BN backward runs its apply
# pass only (gkg_bn_bwd_apply_from_sums); the block driver additionally stores a Grapher's dx channel-major from the GEMM
# (gkg_linear_dgrad_x6_nchw).  Off (the stand-alone statistics launch) under GKG_DETERMINISTIC, SyncBN, frozen / eval-mode BN, an
# active DropPath scale, 2 nb C beyond the scratch, and GKG_DISABLE=bwd_fuse.  The statistics' fp32 partial sums follow the
# producer's partition of the rows: results agree with the two-pass form to rounding (tests/test_hip_bwd_pass_fusion.py).
BWD_FUSE = "bwd_fuse" not in _DISABLED


# Round 9: the same trade for the layers whose upstream gradient an input-gradient GEMM writes — the BN_EPILOGUE link above,
# attached at EVERY size and served by gkg_linear_dgrad_x6_bnbwd_sk (the short-matrix body's epilogue carries the statistics too,
# a residual is added in front of them, dx keeps the bits of the plain call): a block's grouped projection (from fc2's input
# gradient) and a label block's FFN fc1 / fc2 (from the FFN fc2 / FFN fc1 input gradients, the latter with the FFN's residual).
# Four stand-alone statistics launches fewer per cfg2 step; off with bwd_fuse, under GKG_DETERMINISTIC, SyncBN, frozen BN, a
# DropPath scale and sums beyond the scratch (the conditions of _bn_link), and with GKG_DISABLE=dgrad_stats — BN_EPILOGUE_MIN_ROWS
# then decides alone, as before.  The block driver folds the same four (GKG_BLOCK_NO_DGRAD_STATS: off).
DGRAD_STATS = BWD_FUSE and "dgrad_stats" not in _DISABLED
# Round 11: the tile-walk form of the 128-row projection kernel, taken by the library where a launch is two rounds of resident
# workgroups (cfg2: the grouped 4 x (10 368 x 160 -> 160) products, forward and input gradient).  GKG_DISABLE=x6_walk: every projection call carries GKG_X6_NO_WALK (the block driver: GKG_BLOCK_NO_X6_WALK).
X6_WALK = "x6_walk" not in _DISABLED


def _x6_flags() -> int:
    """The per-call ``flags`` of the projection entry points from the module switches."""
    return 0 if X6_WALK else _lib.X6_NO_WALK


def _block_flags() -> int:
    """GkgGrapherBlock / GkgLabelBlock.bwd_flags from the module switches."""
    return ((0 if BWD_FUSE else _lib.BLOCK_NO_BWD_FUSE)
            | (0 if (BWD_FUSE and DGRAD_STATS and BN_EPILOGUE) else _lib.BLOCK_NO_DGRAD_STATS)
            | (0 if X6_WALK else _lib.BLOCK_NO_X6_WALK))


def _bwd_fuse_ok(mean, sync, scale, nb, co) -> bool:
    return (BWD_FUSE and mean is not None and sync is None and scale is None and not DETERMINISTIC and nb == 1
            and _BnScratch.fits(2 * co))


_MR_BN_OK = {}


def _mr_bn_supported(lib, B, G, c, N, M, k, mode, ak, self_graph, flags) -> bool:
    key = (B, G, c, N, M, k, mode, ak, self_graph, flags)
    ok = _MR_BN_OK.get(key)
    if ok is None:
        ok = _MR_BN_OK[key] = bool(lib.gkg_mr_bwd_tm_bnstats_supported(B, G, c, N, M, k, mode, ak, 1 if self_graph else 0, flags))
    return ok


def _mr_bwd(lib, g, nn_idx, arg, B, G, C, N, M, k, mode, ak, has_src, xshape, link):
    """The aggregation's backward -> (gx viewed as ``xshape``, gsrc).  ``link``: the _BnLink of the layer that produced the
    aggregation's input (found on that tensor in the forward) — the scatter then also takes that layer's BN backward statistics
    and leaves them on the link, exactly like _dgrad_x6_with_link."""
    gx = torch.empty((B, N, C), dtype=_F32, device=g.device)
    gsrc = torch.empty((B, M, C), dtype=_F32, device=g.device) if has_src else None
    flags = _mr_bwd_flags()
    if (link is not None and BWD_FUSE and not DETERMINISTIC and link.nb == 1 and link.act == 0 and link.co == C and link.R == B * N
            and _mr_bn_supported(lib, B, G, C // G, N, M, k, mode, ak, not has_src, flags)):
        scratch = _BnScratch.of(g.device)
        with scratch.scoped(lib, 2 * C) as (cur, other, zero):
            _lib.check(lib.gkg_mr_bwd_tm_bnstats(_ptr(g), _ptr(nn_idx), _ptr(arg), _ptr(gx), _ptr(gsrc), B, G, C // G, N, M, k, mode, ak,
                                                 flags, _ptr(link.Y), _ptr(link.mean), _ptr(link.invstd), _ptr(cur), _stream()),
                       "gkg_mr_bwd_tm_bnstats")
        gxv = gx.view(xshape)
        scratch.hand_off(link, gxv, cur, other, zero)
        return gxv, gsrc
    _lib.check(lib.gkg_mr_bwd_tm(_ptr(g), _ptr(nn_idx), _ptr(arg), _ptr(gx), _ptr(gsrc), B, G, C // G, N, M, k, mode, ak, flags, _stream()),
               "gkg_mr_bwd_tm")
    return gx.view(xshape), gsrc


def _bn_link(out, state, meta, scale):
    """Hang a _BnLink on a token-major fp32 layer output (train-mode, rank-local statistics, atomics allowed).  ``state``: the
    layer's (Y, a, c, mean, invstd); ``meta``: (act, nb, co, R, sync[, bn, bias]), what its node keeps as ``ctx.bn``."""
    nb, co, R, sync = meta[1:5]
    if (BN_EPILOGUE and (R >= BN_EPILOGUE_MIN_ROWS or (BWD_FUSE and DGRAD_STATS)) and state[3] is not None and sync is None
            and scale is None and not DETERMINISTIC and out.dtype == _F32 and _BnScratch.fits(2 * nb * co)):
        link = out._gkg_bn_link = _BnLink(*state, *meta)
        return link
    return None


def _layer_of(ctx, state):
    """A node's BN layer for its backward: the link its forward hung on the output, else a record of the saved tensors."""
    return ctx.link if ctx.link is not None else _BnLink(*state, *ctx.bn)


def _dgrad_with_link_ok(lib, R, cin, has_res) -> bool:
    """Whether the statistics-carrying input gradient takes this call (a residual needs the short-matrix body)."""
    return bool(lib.gkg_linear_dgrad_x6_bnbwd_sk_supported(R, cin, 1 if has_res else 0, 1, 0))


def _dgrad_x6_with_link(lib, dY, pd, R, cin, cout, link, residual=None):
    """dx = dY W (+ residual) on the x6 kernel with the producer's BN backward statistics in the epilogue -> dx (the bits of
    _dgrad_x6); leaves the sums on the link."""
    scratch = _BnScratch.of(dY.device)
    with scratch.scoped(lib, 2 * link.nb * link.co) as (cur, other, zero):
        dx = torch.empty((R, cin), dtype=_F32, device=dY.device)
        ws = _sk_ws(dY.device)
        _lib.check(lib.gkg_linear_dgrad_x6_bnbwd_sk(_ptr(dY), cout, _ptr(pd), _ptr(dx), R, cin, cout, _ptr(residual), _ptr(link.Y),
                                                    _ptr(link.a), _ptr(link.c), _ptr(link.mean), _ptr(link.invstd), _ptr(cur),
                                                    link.nb, link.co, link.act, _ptr(ws), ws.numel(), _x6_flags(), _stream()),
                   "gkg_linear_dgrad_x6_bnbwd_sk")
    scratch.hand_off(link, dx, cur, other, zero)      # the other buffer's clear is deferred to the producer's apply pass
    return dx


def _bn_scale_in_kernel(sync, nb, C) -> bool:
    """The ``atomic`` flag of a layer's backward (bn_passes.backward), asked once per node: the two-launch fp64-atomic form on the
    scratch pair — whose kernels can apply a per-image gradient scale (DropPath) themselves instead of a separate elementwise
    launch in front of them (22 launches, 0.6 ms of the cfg4 step) — rather than the two-stage workspace form."""
    return (sync is None or GEMM_MATH == "x6") and not DETERMINISTIC and _BnScratch.fits(2 * nb * C)


class _LinearBNAct(torch.autograd.Function):
    """out = act(BN(x @ W^T + b)) (+ residual), token-major.  ``nchw``: write the result (and read the
    residual) in (B, C, N) layout — the block's last layer."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, residual, bn, act, nchw, out_lowp=False, w16=None, scale=None,
                rows_per_scale=0, want16=False, alias=False, dual=False, xm=None, knn=None, t16=None):
        """``t16`` = (kind, conv) — a row of linear_bf16.KINDS and the projection's module (travels like ``w16``) —, handed over by ``_lin`` only
        where GKG_ENABLE=train_bf16 / train_f16 takes the layer (_train_16bit, asked there: in here gradients are switched off and
        the backward runs outside autocast): the module's cached fragment arrays of that kind are what the own 16-bit products of
        this node's forward and backward stream.
        ``alias``: also return ``x`` itself as a second output (a view).  A caller that uses the layer's input again
        as the residual of a later layer takes the alias for that: both gradient contributions then arrive at THIS node
        and the input-gradient GEMM adds the residual one in its epilogue (``addmm``), instead of autograd summing two
        tensors with a stand-alone add kernel.
        ``dual`` (with ``nchw``, fp32, no DropPath scale): ``residual`` is given TOKEN-MAJOR (R, cout) and the result is
        returned in both layouts, ``(out (B, C, H, W), out_tm (R, cout))`` — see DUAL_LAYOUT below.
        ``xm`` = (B, N) (fp32 token-major output, no residual): the result is written into the x half of a fresh XM operand
        buffer (R, 2 cout) and returned as its (B, N, 4, cout / 4) view (see _xm_xview) — a Grapher's fc1, whose output the
        aggregation and the grouped projection read in place.  ``knn`` (a KnnProblem, with ``xm``): the k-NN problem whose queries
        this output is — the BN-apply pass then also leaves the queries' normalised copies in that call's workspace
        (gkg_bn_apply_knn_prep) and the returned view carries the problem (KnnProblem.mark): no token-preparation launch
        downstream."""
        lib = _lib.load()
        R, cin = x.shape
        cout = weight.shape[0]
        # the layer that produced x (see _BnLink); with ``alias`` the input gradient carries the alias's too (DGRAD_STATS)
        prev = None if (alias and not (BWD_FUSE and DGRAD_STATS)) else getattr(x, "_gkg_bn_link", None)
        group = _sync_group(bn)
        x6f, x6d = _x6(x, weight, bn, 1, "fwd", group), _x6(x, weight, bn, 1, "dgrad", group)
        own = x6f
        taken = None
        pf, pd = _planes(lib, weight, 1, cout, cin, x6f, x6d) if x6f or x6d else (None, None)
        pf, pd = (pf if x6f else None), (pd if x6d else None)
        res = None if residual is None else residual.contiguous()
        ochunk, ldo = 0, cout
        if xm is not None:
            assert nchw is None and not out_lowp and not want16 and residual is None and not dual and cout % 16 == 0
            dt, code = _F32, _lib.F32
            out = torch.empty((R, 2 * cout), dtype=_F32, device=x.device)       # XM: x chunks now, m chunks by the aggregation
            ochunk, ldo = cout // 4, 2 * cout
        elif nchw is None:
            dt, code = _tm_dtype(out_lowp)
            out = torch.empty((R, cout), dtype=dt, device=x.device)
        else:
            assert act == 0
            dt, code = _F32, _lib.F32
            out = torch.empty(nchw, dtype=_F32, device=x.device)
        if own:
            x = x.contiguous()
        sync = None
        out_tm = None
        if dual:
            assert nchw is not None and scale is None and res is not None and res.shape == (R, cout) and res.dtype == _F32
            out_tm = torch.empty((R, cout), dtype=_F32, device=x.device)
        fused_apply = own and _derive_ok(bn, 1, cout, code, want16, group)
        if own and not fused_apply and group is not None:
            own = False                               # exchanged statistics reach the x6 forward through the derive form only
        # this call's apply pass is also the producer of ``knn``'s prepared tokens (knn_prep.py): fc1's queries into the XM buffer, or
        # a Grapher's last layer as the producer of the label graph's keys
        prep = knn if (knn is not None and act == 0 and scale is None
                       and ((xm is not None and not knn.as_keys) or (dual and knn.as_keys))) else None
        if fused_apply:                               # projection (statistics epilogue) -> apply from the sums: 2 launches
            dest = (res, out, ldo, 0, ochunk, act, 0 if nchw is None else nchw[0], scale, rows_per_scale)
            Y, a, c, mean, invstd, sync = _project_apply(lib, x, pf, (R, cin, cout, 1), bias, bn, group, dest, out_tm, prep)
        elif own:                                     # projection kernel with the BN statistics in its epilogue
            Y, a, c, mean, invstd = _linear_fwd_own(lib, x, pf, (R, cin, cout, 1), bias, bn)
        else:
            # bf16 / fp16 autocast with gradients, opt-in: the product on the own kernel of that kind (fp32 A operand rounded on its
            # way into LDS).  The backward runs outside autocast: the decision is recorded here
            taken = t16
            Y = _mm_t(x, weight.view(cout, cin), w16) if taken is None else train16_fwd(taken[0], x, taken[1])
            a, c, mean, invstd, sync = bn_passes.forward_params(lib, Y, bn, bias, R, cout, 1, group)
        if not fused_apply and not (own and mean is None and code == _lib.F32 and not want16):
            prep = None      # besides the train-mode pass only a frozen layer's affine behind the x6 projection, fp32 out, prepares
        if fused_apply:
            pass
        elif prep is not None:                        # the folded affine is also the k-NN's token preparation
            _lib.check(lib.gkg_affine_knn_prep(_ptr(Y), _ptr(a), _ptr(c), *prep.producer_args(lib, out, out_tm, res, ldo, ochunk),
                                               _stream()), "gkg_affine_knn_prep")
        elif nchw is None and want16 and code == _lib.F32:
            # bf16 inference, channels-last chain: also emit the bf16 rounding the next block's first GEMM reads
            out16 = torch.empty((R, cout), dtype=torch.bfloat16, device=x.device)
            _lib.check(lib.gkg_affine_act_dual(_ptr(Y), _ptr(a), _ptr(c), _ptr(res), _ptr(out), _ptr(out16), R, cout, act,
                                               _ptr(scale), rows_per_scale, _stream()), "gkg_affine_act_dual")
            out._gkg_bf16_tm = out16
        elif nchw is None:
            _lib.check(lib.gkg_affine_act(_ptr(Y), _ptr(a), _ptr(c), _ptr(res), _ptr(out), R, cout, 1, ldo, 0, ochunk, act,
                                          code, _ptr(scale), rows_per_scale, _stream()), "gkg_affine_act")
        elif dual:
            _lib.check(lib.gkg_tm_affine_to_nchw_dual(_ptr(Y), _ptr(a), _ptr(c), _ptr(res), _ptr(out), _ptr(out_tm), nchw[0], cout,
                                                      R // nchw[0], _stream()), "gkg_tm_affine_to_nchw_dual")
        else:
            _lib.check(lib.gkg_tm_affine_to_nchw(_ptr(Y), _ptr(a), _ptr(c), _ptr(res), _ptr(out), nchw[0], cout,
                                                 R // nchw[0], _ptr(scale), _stream()), "gkg_tm_affine_to_nchw")
        state = (Y, a, c, mean, invstd)
        ctx.save_for_backward(x, weight, *state)
        # what the backward's layer record (_layer_of) takes behind the saved tensors; eval-mode BN: it reads the running statistics
        ctx.bn = (act, 1, cout, R, sync) + ((bn, bias) if mean is None else ())
        ctx.dual = dual
        ctx.meta = (nchw, residual is not None)
        ctx.scale = (scale, rows_per_scale)
        ctx.gparams = (weight, gamma, beta)
        ctx.pd = pd
        ctx.t16 = taken
        ctx.prev = prev if (prev is not None and pd is not None and prev.nb * prev.co == cin and prev.R == R) else None
        ctx.link = _bn_link(out, state, ctx.bn, scale) if (nchw is None and xm is None) else None
        if xm is not None:
            out = _xm_xview(out, xm[0], xm[1], cout)
            if act == 0 and out.dtype == _F32 and _bwd_fuse_ok(mean, sync, scale, 1, cout):
                # the aggregation behind this layer takes its BN backward statistics in its scatter (_mr_bwd)
                ctx.link = out._gkg_mr_bn_link = _BnLink(*state, *ctx.bn)
            if prep is not None:
                prep.mark(out)                        # the queries' prepared copies are in prep.ws (knn_prep.consumer_ws_flags)
        if alias:
            ctx.set_materialize_grads(False)
            return out, x.view_as(x)
        if dual:
            ctx.set_materialize_grads(False)
            if prep is not None:
                prep.mark(out_tm)                     # the label graph's keys are prepared in prep.ws (grapher_label_forward)
            return out, out_tm
        return out

    @staticmethod
    def backward(ctx, dout, dalias=None):
        lib = _lib.load()
        x, weight, *state = ctx.saved_tensors
        nchw, has_res = ctx.meta
        dtm = None
        if ctx.dual:
            dtm, dalias = dalias, None
            if dout is None and dtm is None:
                return (None,) * 19
        elif dout is None:                                 # only the alias was used downstream
            return (dalias,) + (None,) * 18
        R, cin = x.shape
        cout = weight.shape[0]
        dres = dout if has_res else None
        row_scale = None
        layer = _layer_of(ctx, state)
        mean, sync = layer.mean, layer.sync
        atomic = _bn_scale_in_kernel(sync, 1, cout)     # asked once: it serves the DropPath decision below and the launch form
        if ctx.dual:
            # the output went out in both layouts: its two upstream gradients are summed while the NCHW one is re-laid out, and
            # the (token-major) residual's gradient is that very sum
            if _bwd_fuse_ok(mean, sync, ctx.scale[0], 1, cout):
                # the re-layout pass is also this BN's backward statistics pass (BWD_FUSE); like the block driver it takes a
                # missing NCHW gradient as zeros, so that both issue the same launches
                if dout is None:
                    dout = torch.zeros(nchw, dtype=_F32, device=dtm.device)
                g = torch.empty((R, cout), dtype=_F32, device=dout.device)
                dout_c, dtm_c = dout.contiguous(), (None if dtm is None else dtm.contiguous())
                bn_passes.relayout_bnstats(lib, dout_c, dtm_c, g, layer, nchw[0])
            elif dout is None:
                g = dtm.contiguous()
            elif dtm is None:
                g = torch.empty((R, cout), dtype=_F32, device=dout.device)
                dout_c = dout.contiguous()
                _lib.check(lib.gkg_nchw_to_tm(_ptr(dout_c), _ptr(g), nchw[0], cout, R // nchw[0], _lib.F32, None, _stream()),
                           "gkg_nchw_to_tm")
            else:
                g = torch.empty((R, cout), dtype=_F32, device=dout.device)
                dout_c, dtm_c = dout.contiguous(), dtm.contiguous()
                _lib.check(lib.gkg_nchw_to_tm_add(_ptr(dout_c), _ptr(dtm_c), _ptr(g), nchw[0], cout, R // nchw[0], _stream()),
                           "gkg_nchw_to_tm_add")
            dres = g
        elif nchw is not None and _bwd_fuse_ok(mean, sync, ctx.scale[0], 1, cout):
            g = torch.empty((R, cout), dtype=_F32, device=dout.device)
            dout_c = dout.contiguous()
            bn_passes.relayout_bnstats(lib, dout_c, None, g, layer, nchw[0])
        elif nchw is not None:
            g = torch.empty((R, cout), dtype=_F32, device=dout.device)
            dout_c = dout.contiguous()           # named: the copy must outlive the launch that reads it
            _lib.check(lib.gkg_nchw_to_tm(_ptr(dout_c), _ptr(g), nchw[0], cout, R // nchw[0], _lib.F32,
                                          _ptr(ctx.scale[0]), _stream()), "gkg_nchw_to_tm")      # DropPath: g * mask / keep
        elif ctx.scale[0] is not None and (mean is None or atomic) and not layer.holds_sums():
            g = dout.contiguous()                # DropPath: the BN-backward kernels scale the gradient per image themselves
            row_scale = (ctx.scale[0].contiguous().float(), ctx.scale[1])
        elif ctx.scale[0] is not None:
            g = (dout.view(-1, ctx.scale[1], cout) * ctx.scale[0].view(-1, 1, 1)).view(R, cout)
        else:
            g = dout.contiguous()                # (an xm output's gradient arrives (B, N, 4, cout / 4): the same memory as (R, cout))
        dY = torch.empty_like(layer.Y)
        dWv, dgamma, dbeta = _grad_outs(ctx.gparams, (cout, cin), cout, dY.device)
        dbias, dgamma, dbeta = bn_passes.backward(lib, layer, g, cout, 0, dY, (dgamma, dbeta), ctx.needs_input_grad[2:5], row_scale,
                                                  atomic)
        W = weight.view(cout, cin)

        def rides(dalias, shape):
            """The alias gradient as the residual of an own input-gradient epilogue (fp32, exactly the product's shape), or None."""
            return dalias if (dalias is not None and dalias.dtype == _F32 and dalias.shape == shape) else None

        if not ctx.needs_input_grad[0]:
            dx = None
        elif ctx.prev is not None and dalias is None:
            dx = _dgrad_x6_with_link(lib, dY, ctx.pd, R, cin, cout, ctx.prev)      # + the producer's BN backward statistics
        # (with the skip gradient only where the short-matrix body runs, i.e. up to 4 096 rows and 640 columns: the tile body's
        # statistics epilogue takes no residual.  Above that this branch is EXPECTED to miss: the plain input gradient below adds
        # the residual, the link stays empty and the producer runs its own statistics pass — as the block driver's
        # dgrad_stats_ok does for the same shapes)
        elif ctx.prev is not None and rides(dalias, (R, cin)) is not None and _dgrad_with_link_ok(lib, R, cin, True):
            dx = _dgrad_x6_with_link(lib, dY, ctx.pd, R, cin, cout, ctx.prev, dalias.contiguous())      # + the skip gradient in front
            dalias = None
        elif ctx.pd is not None:
            dx = torch.empty((R, cin), dtype=_F32, device=dY.device)
            res = rides(dalias, dx.shape)
            res = None if res is None else res.contiguous()
            _dgrad_x6(lib, dY, cout, R * cout, ctx.pd, dx, R, cin, cout, 1, res)
            if res is not None:
                dalias = None
        elif ctx.t16 is not None:                          # GKG_ENABLE=train_bf16 / train_f16: the own product, the skip gradient in its epilogue
            res = rides(dalias, (R, cin))
            dx = train16_dgrad(ctx.t16[0], dY, ctx.t16[1], residual=res)
            if res is not None:
                dalias = None
        elif dalias is not None and dalias.dtype == dY.dtype:
            dx = torch.addmm(dalias, dY, W)                # the residual-path gradient rides in the GEMM epilogue
            dalias = None
        else:
            dx = torch.mm(dY, W)
        if dalias is not None and dx is not None:
            dx = dx + dalias
        elif dalias is not None:
            dx = dalias
        if ctx.t16 is not None and ctx.t16[0].own_wgrad:
            # launched from the node: the deferred weight-gradient queue's problem records are x6 problems
            dW = linear_bf16_wgrad(dY, x, dWv).view_as(weight)
        else:                                              # (a kind without a weight-gradient kernel of its own: the path of the switch-off run)
            dW = _wgrad(dY, x, dWv).view_as(weight)
        return dx, dW, dbias, dgamma, dbeta, dres, None, None, None, None, None, None, None, None, None, None, None, None, None


class _GroupedLinearBNAct(torch.autograd.Function):
    """The reference's BasicConv: Conv2d(1x1, groups=4) + BN + act on the interleaved [x, m] channels (torch_nn.py:57-69 behind
    torch_vertex.py:57-61), reading the XM operand buffer (R, 4 ci) instead of an interleaved tensor: group q's ci inputs are
    the contiguous columns [q ci, (q+1) ci) = [x chunk | m chunk]; the weight's input columns are taken in that order (x6 planes
    built with kperm, or _kperm_weight for the library paths).  -> out (R, 4 co) token-major (column q co + j).  ``t16``: the
    caller's _train_grouped_16bit decision, (kind, conv) or None — the product and the input gradient on the own grouped 16-bit kernel
    (taken where the x6 kernels refuse: under autocast)."""

    @staticmethod
    def forward(ctx, XM, weight, bias, gamma, beta, bn, act, out_lowp=False, w16=None, t16=None):
        lib = _lib.load()
        nb = 4
        R, ci = XM.shape[0], XM.shape[1] // nb
        XM = XM.contiguous()
        U = XM.view(R, nb, ci).permute(1, 0, 2)                     # (nb, R, ci): strides (ci, 4 ci, 1)
        cout = weight.shape[0]
        co = cout // nb
        Wg = weight.view(nb, co, ci)
        group = _sync_group(bn)
        x6f, x6d = _x6(U, weight, bn, nb, "fwd", group) and act == 1, _x6(U, weight, bn, nb, "dgrad", group)
        own = x6f                                                   # (the fp32-MFMA forward kernel takes no operand pitch)
        pf, pd = _planes(lib, weight, nb, co, ci, x6f, x6d, kperm=1) if x6f or x6d else (None, None)
        pf, pd = (pf if x6f else None), (pd if x6d else None)
        dt, code = _tm_dtype(out_lowp)
        out = torch.empty((R, cout), dtype=dt, device=XM.device)
        sync = None
        fused_apply = own and _derive_ok(bn, nb, co, code, False, group)
        if own and not fused_apply and group is not None:
            own = False
        if fused_apply:
            Y, a, c, mean, invstd, sync = _project_apply(lib, U, pf, (R, ci, co, nb), bias, bn, group,
                                                         (None, out, cout, co, 0, act, 0, None, 0))
        elif own:
            Y, a, c, mean, invstd = _linear_fwd_own(lib, U, pf, (R, ci, co, nb), bias, bn)
        else:
            if t16 is not None:                                     # GKG_ENABLE=train_grouped: one launch, no gathered copy, fp32 Y
                Y = train16_grouped_fwd(t16[0], XM, t16[1])         # (nb, R, co)
            elif XM.dtype == torch.bfloat16:
                Wb = weight.to(torch.bfloat16) if w16 is None else w16
                Y = torch.bmm(U, _kperm_weight(Wb.view(nb, co, ci)).transpose(1, 2), out_dtype=_F32)
            else:
                Y = torch.bmm(U, _kperm_weight(Wg).transpose(1, 2))        # (nb, R, co)
                if Y.dtype != _F32:
                    Y = Y.float()
            a, c, mean, invstd, sync = bn_passes.forward_params(lib, Y, bn, bias, R, co, nb, group)
        if not fused_apply:
            _lib.check(lib.gkg_affine_act(_ptr(Y), _ptr(a), _ptr(c), None, _ptr(out), R, co, nb, cout, co, 0, act,
                                          code, None, 0, _stream()), "gkg_affine_act")
        state = (Y, a, c, mean, invstd)
        ctx.save_for_backward(XM, weight, *state)
        ctx.bn = (act, nb, co, R, sync) + ((bn, bias) if mean is None else ())
        ctx.gparams = (weight, gamma, beta)
        ctx.pd = pd
        ctx.t16 = t16                                               # (the backward runs outside autocast: the decision is the forward's)
        ctx.link = _bn_link(out, state, ctx.bn, None)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        XM, weight, *state = ctx.saved_tensors
        layer = _layer_of(ctx, state)
        nb = 4
        R, ci = XM.shape[0], XM.shape[1] // nb
        cout = weight.shape[0]
        co = cout // nb
        g = dout.contiguous()
        dY = torch.empty_like(layer.Y)
        dWv, dgamma, dbeta = _grad_outs(ctx.gparams, (nb, co, ci), cout, dY.device)
        dbias, dgamma, dbeta = bn_passes.backward(lib, layer, g, cout, co, dY, (dgamma, dbeta), ctx.needs_input_grad[2:5], None,
                                                  _bn_scale_in_kernel(layer.sync, nb, co))
        Wg = weight.view(nb, co, ci)
        if not ctx.needs_input_grad[0]:
            dXM = None
        elif ctx.pd is not None:                                    # dXM (R, 4 ci) written in place: [direct chunk | dm chunk] per group
            dXM = torch.empty((R, nb * ci), dtype=_F32, device=dY.device)
            _dgrad_x6(lib, dY, co, R * co, ctx.pd, dXM, R, ci, co, nb, ldx=nb * ci, x_bs=ci)
        elif ctx.t16 is not None:                                   # dXM written in place by the own grouped kernel: no re-layout copy
            dXM = train16_grouped_dgrad(ctx.t16[0], dY, ctx.t16[1])
        else:
            dXM = torch.bmm(dY, _kperm_weight(Wg)).permute(1, 0, 2).reshape(R, nb * ci)
        dW = _wgrad_grouped(dY, XM.view(R, nb, ci).permute(1, 0, 2), dWv, kperm=1).view_as(weight)
        return dXM, dW, dbias, dgamma, dbeta, None, None, None, None, None


# ----------------------------------------------------------------------------------------------- BN (+ act) behind a library conv
# The backbone's stem and downsample layers are 3x3 convolutions (MIOpen) followed by BN (+ GELU) (reference gkgnet.py:74-118).
# On channels-last tensors their output IS a token-major matrix, so the BN (+ activation) runs on the same bandwidth kernels
# as inside the blocks (statistics at 6-7 TB/s, one apply pass with the fast-erf GELU, two-pass backward) instead of
# MIOpenBatchNorm{Fwd,Bwd}Spatial + stand-alone GELU kernels: 6.2 + 1.2 ms of the 92.7 ms GKGNet-576 train step (round 3).
STEM_BN = True               # (a module constant the A/B tests flip; no environment switch)


class _BNActTM(torch.autograd.Function):
    """out (T, C) = act(BN(Y)) for a token-major matrix Y (train-mode batch statistics or eval-mode running statistics)."""

    @staticmethod
    def forward(ctx, Y, gamma, beta, bn, act):
        lib = _lib.load()
        R, C = Y.shape
        a, c, mean, invstd, sync = bn_passes.forward_params(lib, Y, bn, None, R, C, 1, _sync_group(bn))
        out = torch.empty_like(Y)
        _lib.check(lib.gkg_affine_act(_ptr(Y), _ptr(a), _ptr(c), None, _ptr(out), R, C, 1, C, 0, 0, act, _lib.F32, None, 0, _stream()),
                   "gkg_affine_act")
        ctx.save_for_backward(Y, a, c, mean, invstd)
        ctx.bn = (act, 1, C, R, sync) + ((bn, None) if mean is None else ())      # (the conv in front owns its bias)
        ctx.gparams = (None, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        layer = _BnLink(*ctx.saved_tensors, *ctx.bn)
        C = layer.co
        g = dout.contiguous()
        dY = torch.empty_like(layer.Y)
        _, dgamma, dbeta = _grad_outs(ctx.gparams, None, C, dY.device)
        _, dgamma, dbeta = bn_passes.backward(lib, layer, g, C, 0, dY, (dgamma, dbeta), (False,) + ctx.needs_input_grad[1:3], None,
                                              _bn_scale_in_kernel(layer.sync, 1, C))
        return dY, dgamma, dbeta, None, None


def bn_act_supported(bn, x, act_mod) -> bool:
    """fp32 CUDA activations in channels-last memory (what a channels-last convolution returns), affine BN, GELU or no
    activation, channel count a multiple of 4.  Train-mode and eval-mode (frozen) BN alike, with or without gradients."""
    if not (ENABLED and STEM_BN and x.is_cuda and x.dim() == 4 and x.dtype == _F32 and _bn_ok(bn)):
        return False
    if act_mod is not None and not isinstance(act_mod, torch.nn.GELU):
        return False
    C = x.shape[1]
    if C % 4 or C > 4096 or not x.permute(0, 2, 3, 1).is_contiguous():
        return False
    return True


def bn_act(x, bn, act_mod):
    """act(BN(x)) for a channels-last (B, C, H, W) tensor, returned channels-last (same values and shape as the reference's
    ``act(norm(x))``, gkgnet.py:81-83,109)."""
    B, C, H, W = x.shape
    Y = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
    out = _BNActTM.apply(Y, bn.weight, bn.bias, bn, 0 if act_mod is None else 1)
    return out.view(B, H, W, C).permute(0, 3, 1, 2)


# ----------------------------------------------------------------------------------------------- the stem's first convolution
# Conv2d(3 -> C1/2, 3x3, stride 2, padding 1) on the image as a direct kernel (csrc/gkg_stem.hip): MIOpen's implicit-GEMM forms
# need 756 us (bf16 autocast) / 1 015 us (fp32) for it at B = 32, 576 x 576.  (STEM_CONV = False: the library call; tests.)
STEM_CONV = True


def conv_bn_act_eval_supported(conv, bn, act_mod, x) -> bool:
    """Inference form of a stem / downsample unit: library convolution (channels-last, no bias) + ONE own pass with the
    eval-mode BN, the conv bias (+ GELU) folded in (fp32, or bf16 autocast)."""
    if not (ENABLED and STEM_BN and x.is_cuda and x.dim() == 4 and not torch.is_grad_enabled()):
        return False
    if not (isinstance(conv, torch.nn.Conv2d) and conv.groups == 1 and conv.padding_mode == "zeros"
            and not isinstance(conv.padding, str) and conv.out_channels % 8 == 0 and conv.weight.dtype == _F32):
        return False
    if not (_bn_ok(bn) and not bn.training and bn.track_running_stats and bn.running_mean is not None):
        return False
    if act_mod is not None and not isinstance(act_mod, torch.nn.GELU):
        return False
    if torch.is_autocast_enabled():
        return torch.get_autocast_dtype("cuda") == torch.bfloat16 and x.dtype in (_F32, torch.bfloat16)
    return x.dtype == _F32


@torch.no_grad()
def conv_bn_act_eval(conv, bn, act_mod, x, want32=True, want16=False):
    """-> channels-last (B, Cout, Ho, Wo): the fp32 result (want32; with the bf16 rounding riding along as ``_gkg_bf16`` for
    the next block's entry when want16) or only its bf16 rounding (want16 alone: the next convolution's operand).  The
    library's separate bias add, its BN kernel, the stand-alone GELU and the layout / cast copies around them (1.4 ms of
    the 22.7 ms GKGNet-576 forward, tools/prof_backbone_ops.py cfg3) become one streaming pass per unit."""
    lib = _lib.load()
    cout = conv.out_channels
    a, c = bn_passes.eval_ac(lib, bn, conv.bias, cout)
    ac16 = torch.is_autocast_enabled()
    dt = torch.bfloat16 if ac16 else _F32
    xin = x if (x.dtype == dt and x.is_contiguous(memory_format=torch.channels_last)) else \
        x.to(dtype=dt, memory_format=torch.channels_last)
    w = derived.w16(conv) if ac16 else conv.weight
    with torch.autocast("cuda", enabled=False):
        y = torch.ops.aten.convolution(xin, w, None, list(conv.stride), list(conv.padding), list(conv.dilation), False, [0, 0], 1)
    if not y.is_contiguous(memory_format=torch.channels_last):
        y = y.contiguous(memory_format=torch.channels_last)
    B, _, Ho, Wo = y.shape
    R = B * Ho * Wo
    act = 0 if act_mod is None else 1
    o32 = torch.empty((B, Ho, Wo, cout), dtype=_F32, device=y.device) if want32 else None
    o16 = torch.empty((B, Ho, Wo, cout), dtype=torch.bfloat16, device=y.device) if want16 else None
    if ac16:
        _lib.check(lib.gkg_affine_act_bf16in(_ptr(y), _ptr(a), _ptr(c), _ptr(o32), _ptr(o16), R, cout, act, _stream()),
                   "gkg_affine_act_bf16in")
    elif want32 and want16:
        _lib.check(lib.gkg_affine_act_dual(_ptr(y), _ptr(a), _ptr(c), None, _ptr(o32), _ptr(o16), R, cout, act, None, 0, _stream()),
                   "gkg_affine_act_dual")
    else:
        out = o32 if want32 else o16
        _lib.check(lib.gkg_affine_act(_ptr(y), _ptr(a), _ptr(c), None, _ptr(out), R, cout, 1, cout, 0, 0, act,
                                      _lib.F32 if want32 else _lib.BF16, None, 0, _stream()), "gkg_affine_act")
    if want32:
        res = o32.permute(0, 3, 1, 2)
        if want16:
            res._gkg_bf16 = (res._version, o16.view(R, cout))
        return res
    return o16.permute(0, 3, 1, 2)


from .stem import _StemConv, _ConvBeforeBN, _AddPosEmbed      # noqa: E402  (autograd Functions of the stem path: stem.py)


def stem_conv_supported(conv, x) -> bool:
    return (ENABLED and STEM_CONV and isinstance(conv, torch.nn.Conv2d) and x.is_cuda and x.dim() == 4 and x.dtype == _F32
            and conv.weight.dtype == _F32 and tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (2, 2)
            and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and conv.padding_mode == "zeros" and x.shape[1] == conv.in_channels
            and bool(_lib.load().gkg_stem_conv3x3s2_supported(conv.in_channels, conv.out_channels)))



def stem_conv(conv, x, bn=None):
    """Training form: the plain convolution (its BN runs on the token-major kernels behind it, fused.bn_act).  ``bn``: the
    BatchNorm directly behind it — in training mode the bias gradient is exactly zero and is not reduced."""
    bn_behind = STEM_BN and isinstance(bn, torch.nn.modules.batchnorm._BatchNorm) and bn_passes.batch_stats(bn)
    return _StemConv.apply(x, conv.weight, conv.bias, bn_behind)



def conv_before_bn(conv, bn, x):
    """``conv(x)`` for a Conv2d directly followed by ``bn``; the lean backward above when that BN normalises with batch
    statistics (training), the module call otherwise."""
    if (ENABLED and STEM_BN and x.is_cuda and x.dtype == _F32 and not torch.is_autocast_enabled() and torch.is_grad_enabled()
            and isinstance(conv, torch.nn.Conv2d) and isinstance(bn, torch.nn.modules.batchnorm._BatchNorm)
            and bn_passes.batch_stats(bn) and conv.groups == 1 and tuple(conv.dilation) == (1, 1)
            and conv.padding_mode == "zeros" and not isinstance(conv.padding, str) and conv.weight.dtype == _F32):
        return _ConvBeforeBN.apply(x, conv.weight, conv.bias, list(conv.stride), list(conv.padding))
    return conv(x)



def add_pos_embed(x, pos):
    if (ENABLED and x.is_cuda and x.dim() == 4 and pos.dim() == 4 and pos.shape[0] == 1 and pos.shape[1:] == x.shape[1:]
            and x.dtype == pos.dtype == _F32 and is_channels_last(x)):
        return _AddPosEmbed.apply(x, pos)
    return x + pos


@torch.no_grad()
def stem_conv_bn_act_eval(conv, bn, act_mod, x, out_bf16: bool):
    """Inference: conv + eval-mode BN (+ GELU) in ONE launch, channels-last output (bf16 under bf16 autocast, like the library
    convolution's output there)."""
    lib = _lib.load()
    B, cin, H, W = x.shape
    cout = conv.out_channels
    a, c = bn_passes.eval_ac(lib, bn, conv.bias, cout)                      # conv bias folded into the shift
    out = torch.empty((B, (H + 1) // 2, (W + 1) // 2, cout), dtype=torch.bfloat16 if out_bf16 else _F32, device=x.device)
    _lib.check(lib.gkg_stem_conv3x3s2_fwd(_ptr(x.contiguous()), _ptr(conv.weight.contiguous()), None, _ptr(a), _ptr(c), _ptr(out), B, cin,
                                          H, W, cout, 0 if act_mod is None else 1, _lib.BF16 if out_bf16 else _lib.F32, _stream()),
               "gkg_stem_conv3x3s2_fwd")
    return out.permute(0, 3, 1, 2)


# ----------------------------------------------------------------------------------------------- graph ops
# Token-major tensors reach the graph kernels as VIEWS (pointer, row pitch, chunk) — include/gkg_hip.h "XM layout".  A Grapher's
# fc1 writes its output x into the x half of the grouped projection's operand buffer XM (T, 2C); that half travels through
# autograd as a (B, N, 4, C/4) tensor with strides (N 2C, 2C, C/2, 1) over the buffer's storage (an alias without a view
# relation: the aggregation fills the m half of the same storage behind autograd's back, which must not bump x's version).
def _alias(t, size, stride, offset=0):
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage(), t.storage_offset() + offset, size, stride)


def _xm_xview(XM, B, N, C):
    """The x half of an XM buffer (B N, 2C) as a (B, N, 4, C/4) tensor."""
    return _alias(XM, (B, N, 4, C // 4), (N * 2 * C, 2 * C, C // 2, 1))


def _is_xm_half(x) -> bool:
    if x.dim() != 4 or x.shape[2] != 4 or x.dtype != _F32:
        return False
    B, N, _, h = x.shape
    return x.stride() == (N * 8 * h, 8 * h, 2 * h, 1) and x.data_ptr() % 16 == 0


def _xm_of(x):
    """The whole XM buffer (B N, 2C) whose x half ``x`` is."""
    B, N, _, h = x.shape
    return _alias(x, (B * N, 8 * h), (8 * h, 1))


def _tm_view(x):
    """(B, N, C, ldx, xchunk) of a token-major tensor: a contiguous (B, N, C) / (B N, C) matrix or the x half of an XM buffer."""
    if _is_xm_half(x):
        B, N, _, h = x.shape
        return B, N, 4 * h, 8 * h, h
    B, N, C = x.shape
    return B, N, C, C, 0


def _as_tokens(x):
    """What a kernel takes as the x pointer: the tensor itself when it is an XM half (read through its view), else contiguous."""
    return x if _is_xm_half(x) else x.contiguous()


from . import knn_prep                          # noqa: E402  (the prepared-token handshake between a BN-apply pass and the k-NN)


def _rp_arg(relative_pos, N, M):
    rp = relative_pos.detach().to(_F32).reshape(-1, relative_pos.shape[-1]).contiguous()
    if tuple(rp.shape) != (N, M):
        raise _lib.GkgError(f"relative_pos must be (1,{N},{M}), got {tuple(relative_pos.shape)}")
    return rp


@torch.no_grad()
def _knn_graph(x, y, relative_pos, k, dilation, G, compact):
    """knn_graph_tm / knn_graph_tm16: the same problem, flags and workspace; ``compact`` chooses the output and the entry point."""
    lib = _lib.load()
    B, N, C, ldx, xchunk = _tm_view(x)
    x = _as_tokens(x)
    c = C // G
    M = N if y is None else y.shape[1]
    rp = None if relative_pos is None else _rp_arg(relative_pos, N, M)
    # (under opt-in bf16 autocast the reference's own x.y^T runs in bf16, and rounds the result to bf16)
    contract = knn_contract()
    flags = knn_prep.problem_flags(relative_pos, contract == "bf16", contract == "f16")
    if compact:
        out, entry = torch.empty((B * G, N, k), dtype=torch.int16, device=x.device), "gkg_knn_fwd_tm16"
        outs = (_ptr(out),)
    else:
        out, entry = torch.empty((2, B * G, N, k), dtype=torch.int64, device=x.device), "gkg_knn_fwd_tm"
        outs = (out[0].data_ptr(), out[1].data_ptr())
    ws, flags = knn_prep.consumer_ws_flags(lib, x, B, G, c, N, M, k, dilation, y is not None, rp is not None, flags, False)
    _lib.check(getattr(lib, entry)(_ptr(x), ldx, xchunk, _ptr(y), _ptr(rp), *outs, B, G, c, N, M, k, dilation, _lib.F32, flags,
                                   _ptr(ws), ws.numel(), _stream()), entry)
    return out


def knn_contract():
    """The opt-in 16-bit contraction the k-NN call made right now would take: "bf16" (KNN_BF16 under bf16 autocast), "f16" (KNN_F16
    under CUDA autocast of either 16-bit dtype; bf16 wins when both apply) or None (the index-exact fp32 contract)."""
    if not ((KNN_BF16 or KNN_F16) and torch.is_autocast_enabled()):
        return None
    dt = torch.get_autocast_dtype("cuda")
    if KNN_BF16 and dt == torch.bfloat16:
        return "bf16"
    return "f16" if KNN_F16 and dt in (torch.bfloat16, torch.float16) else None


def knn_graph_tm(x, y, relative_pos, k, dilation, G):
    """x (B,N,C) [or the x half of an XM buffer], y (B,M,C)|None token-major -> edge_index (2, B*G, N, k) int64."""
    return _knn_graph(x, y, relative_pos, k, dilation, G, False)


_KNN_GRAPH_TM = knn_graph_tm             # the library's own function (tests patch ``fused.knn_graph_tm`` to record / force graphs)

# Compact graph inside the block (round 5): a Grapher discards its graph (reference torch_vertex.py:330), so between the k-NN
# and the aggregation launches the neighbour lists travel as u16 rows (B*G, N, k) — no int64 plane, no centre plane (GKGNet-576
# stage 1: 24 MB written per launch instead of 191 MB; pvig_m stage 1: 170 MB instead of 1.36 GB).  Same neighbours, same bits.
# Taken when nobody asked for the edge_index, M <= 65536 and ``fused.knn_graph_tm`` is the library's own function (tests that
# record or force graphs patch it and get the int64 form).  GKG_DISABLE=knn_compact: off.
KNN_COMPACT = "knn_compact" not in _DISABLED


def knn_graph_tm16(x, y, relative_pos, k, dilation, G):
    """x (B,N,C) [or the x half of an XM buffer], y (B,M,C)|None token-major -> neighbour lists (B*G, N, k) int16 (the bits of u16 rows)."""
    return _knn_graph(x, y, relative_pos, k, dilation, G, True)


def _xm_out(x, B, N, C, dt):
    """The operand buffer a mode-1 aggregation writes: the buffer ``x`` already lives in (only m is written then), else a fresh one."""
    if _is_xm_half(x) and dt == _F32:
        return _xm_of(x)
    return torch.empty((B * N, 2 * C), dtype=dt, device=x.device)


class _MaxRelativeTM(torch.autograd.Function):
    """mode 0: m (B, N, C); mode 1: the grouped projection's operand buffer XM (B N, 2C) (x may be its x half already)."""

    @staticmethod
    def forward(ctx, x, src, nn_idx, G, mode, out_lowp=False):
        lib = _lib.load()
        B, N, C, ldx, xchunk = _tm_view(x)
        x = _as_tokens(x)
        M = N if src is None else src.shape[1]
        k = nn_idx.shape[2]
        dt, code = _tm_dtype(out_lowp)
        out = _xm_out(x, B, N, C, dt) if mode == 1 else torch.empty((B, N, C), dtype=dt, device=x.device)
        need = any(ctx.needs_input_grad[:2])
        ak = 1 if M <= 65536 else 0              # the winning neighbour's row index (u16) instead of its slot (u8)
        arg = torch.empty((B, N, C), dtype=torch.int16 if ak else torch.uint8, device=x.device) if need else None
        if nn_idx.dtype == torch.int16:          # compact lists (knn_graph_tm16; M <= 65536, so ak == 1: the backward needs no index)
            _lib.check(lib.gkg_mr_fwd_tm16(_ptr(x), ldx, xchunk, _ptr(src), _ptr(nn_idx), _ptr(out), _ptr(arg), B, G, C // G, N, M, k,
                                           mode, code, ak, _stream()), "gkg_mr_fwd_tm16")
            nn_idx = None
        else:
            _lib.check(lib.gkg_mr_fwd_tm(_ptr(x), ldx, xchunk, _ptr(src), _ptr(nn_idx), _ptr(out), _ptr(arg), B, G, C // G, N, M, k,
                                         mode, code, ak, _stream()), "gkg_mr_fwd_tm")
        ctx.save_for_backward(nn_idx, arg)
        ctx.meta = (B, G, C, N, M, k, mode, src is not None, ak, tuple(x.shape))
        ctx.bn_link = getattr(x, "_gkg_mr_bn_link", None) if (need and mode == 1) else None      # see _mr_bwd
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        nn_idx, arg = ctx.saved_tensors
        B, G, C, N, M, k, mode, has_src, ak, xshape = ctx.meta
        g = g.contiguous()
        gxv, gsrc = _mr_bwd(lib, g, nn_idx, arg, B, G, C, N, M, k, mode, ak, has_src, xshape, ctx.bn_link)
        return gxv, gsrc, None, None, None, None


# ----------------------------------------------------------------------------------------------- row g2: k-NN + aggregation
# ONE kernel builds the graph and consumes it (csrc/gkg_knn_tile.h, MRF): the workgroup that has merged the lists of its 64
# queries gathers their neighbour rows and writes m into the grouped projection's operand buffer, plus the winning rows; no
# (2, B*G, N, k) int64 edge_index, no centre plane, no mr_fwd launch (reference torch_edge.py:164-176 -> torch_vertex.py:49-61).
# Taken for fp32 training / inference blocks whose graph runs on the fp32 tile kernel with merged per-wave lists
# (gkg_knn_mr_fused_supported: the 18 x 18 stages and the label graphs over them; key-split and prefilter shapes keep the two
# launches) — and only while ``fused.knn_graph_tm`` is the library's own function: tests that record or force graphs patch
# it and thereby select the two-launch form.  GKG_DISABLE=knn_mr: off.
KNN_MR = "knn_mr" not in _DISABLED


class _KnnMaxRelativeTM(torch.autograd.Function):
    """(XM (B N, 2C), edge_index (2, B*G, N, k) | empty) = aggregation over the k-NN graph of x (B, N, C) [keys / values src (B, M, C)]."""

    @staticmethod
    def forward(ctx, x, src, relative_pos, k, d, G, want_nn):
        lib = _lib.load()
        B, N, C, ldx, xchunk = _tm_view(x)
        x = _as_tokens(x)
        M = N if src is None else src.shape[1]
        c = C // G
        rp = None if relative_pos is None else _rp_arg(relative_pos, N, M)
        flags = knn_prep.problem_flags(relative_pos)
        XM = _xm_out(x, B, N, C, _F32)
        arg = torch.empty((B, N, C), dtype=torch.int16, device=x.device)
        # the (2, B*G, N, k) int64 edge_index only for callers that return the graph (GrapherLabel / tests): written by the kernel
        edge = torch.empty((2, B * G, N, k) if want_nn else (0,), dtype=torch.int64, device=x.device)
        ws, flags = knn_prep.consumer_ws_flags(lib, x, B, G, c, N, M, k, d, src is not None, rp is not None, flags, True)
        _lib.check(lib.gkg_knn_mr_fwd_tm(_ptr(x), ldx, xchunk, _ptr(src), _ptr(rp), _ptr(XM), _ptr(arg), None,
                                         edge[0].data_ptr() if want_nn else None, edge[1].data_ptr() if want_nn else None, B, G, c,
                                         N, M, k, d, flags, _ptr(ws), ws.numel(), _stream()), "gkg_knn_mr_fwd_tm")
        ctx.save_for_backward(arg)
        ctx.meta = (B, G, C, N, M, k, src is not None, tuple(x.shape))
        ctx.bn_link = getattr(x, "_gkg_mr_bn_link", None)                  # see _mr_bwd
        ctx.mark_non_differentiable(edge)
        ctx.set_materialize_grads(False)          # (no zero-filled int64 "gradient" of the graph output: 4.8 us per step)
        return XM, edge

    @staticmethod
    def backward(ctx, g, _gnn=None):
        lib = _lib.load()
        (arg,) = ctx.saved_tensors
        B, G, C, N, M, k, has_src, xshape = ctx.meta
        if g is None:
            return (None,) * 7
        g = g.contiguous()
        gxv, gsrc = _mr_bwd(lib, g, None, arg, B, G, C, N, M, k, 1, 1, has_src, xshape, ctx.bn_link)
        return gxv, gsrc, None, None, None, None, None


def _knn_ahead_ok() -> bool:
    """The k-NN problem of a call can be told before its tokens exist (the fused kernel chosen, the tokens prepared by their
    producer): not with the bf16 / fp16 contraction, nor with a patched ``knn_graph_tm`` (tests that record or force graphs)."""
    return knn_graph_tm is _KNN_GRAPH_TM and not ((KNN_BF16 or KNN_F16) and torch.is_autocast_enabled())


def _knn_mr_shapes_ok(B, N, C, M, has_src, relative_pos, k, d, G, nn_, lp) -> bool:
    """The shape / mode part of _knn_mr_ok (what is known before the tensors exist: fc1 asks on behalf of its output)."""
    if not (KNN_MR and not lp and _knn_ahead_ok()):
        return False
    if C % 16 or M > 65536 or len(nn_) != 3:
        return False
    return bool(_lib.load().gkg_knn_mr_fused_supported(B, G, C // G, N, M, k, d, 1 if has_src else 0,
                                                       0 if relative_pos is None else 1, knn_prep.problem_flags(relative_pos)))


def _knn_mr_ok(x, src, relative_pos, k, d, G, nn_, lp) -> bool:
    """The fused k-NN + aggregation kernel applies (see KNN_MR)."""
    if not (x.dtype == _F32 and (x.is_contiguous() or _is_xm_half(x)) and (src is None or (src.dtype == _F32 and src.is_contiguous()))):
        return False
    B, N, C, _, _ = _tm_view(x)
    M = N if src is None else src.shape[1]
    return _knn_mr_shapes_ok(B, N, C, M, src is not None, relative_pos, k, d, G, nn_, lp)


def _knn_key_for(B, N, C, M, has_src, relative_pos, gc, groups, lp, want_edge, lp_prep=False):
    """The KnnProblem of the k-NN call _graph_and_project will make for these shapes (fc1 prepares its queries), or None when the
    queries cannot be prepared ahead (_knn_ahead_ok) or by the preparation kernel — which takes group widths that are multiples
    of 4 (the block driver never asks: block.grapher_ok excludes that shape before).  bf16 inference (``lp``) prepares only
    inside the own bf16 projection's launch (``lp_prep``: GKG_ENABLE=lin_bf16,lin_bf16_prep on the channels-last chain)."""
    if (lp and not lp_prep) or not _knn_ahead_ok() or (C // groups) % 4:
        return None
    fused_mr = _knn_mr_shapes_ok(B, N, C, M, has_src, relative_pos, gc.k, gc.d, groups, gc.gconv.nn, lp)
    return knn_prep.KnnProblem(B, groups, C // groups, N, M, gc.k, gc.d, has_src, relative_pos, fused_mr)


def _aggregate_project(x1b, yb, nn_idx, groups, nn_, C, lp):
    """MRConv2d.forward on token-major tensors -> (T, 2C): the fused launch where it applies, else aggregation kernel +
    grouped projection."""
    if _mr_gemm_ok(nn_, C, lp):                                     # row g1, bf16 inference: one launch
        return mr_grouped_linear_eval(x1b, yb, nn_idx, groups, nn_[0], nn_[1])
    XM = _MaxRelativeTM.apply(x1b, yb, nn_idx, groups, 1, lp)       # (T, 2C) operand buffer [x | m]
    return _GroupedLinearBNAct.apply(XM, nn_[0].weight, nn_[0].bias, nn_[1].weight, nn_[1].bias, nn_[1], 1, lp,
                                     derived.w16(nn_[0]) if lp else None, _train_grouped_16bit(XM, nn_[0], nn_[1]))   # (T, 2C)


# ----------------------------------------------------------------------------------------------- row g1 (inference)
# bf16 inference: gather + max-relative + interleave + grouped 1x1 projection + BN(eval) + GELU in ONE launch
# (csrc/gkg_mrgemm.hip) — the [x, m] operand is produced tile by tile in LDS and never written.  GKG_DISABLE=mr_gemm restores
# the three-launch form (gkg_mr_fwd_tm -> batched GEMM -> gkg_affine_act).
MR_GEMM = "mr_gemm" not in _DISABLED


def _mr_gemm_ok(nn_, C, lp) -> bool:
    conv, bn = nn_[0], nn_[1]
    return (MR_GEMM and lp and not bn.training and bn.track_running_stats and conv.groups == 4 and C % 16 == 0 and C <= 768
            and conv.weight.shape[0] == 2 * C and conv.weight.shape[1] == C // 2)


@torch.no_grad()
def mr_grouped_linear_eval(x, src, nn_idx, G, conv, bn, act=1):
    """x (B, N, C) fp32, src (B, M, C) fp32 | None, nn_idx (B*G, N, k) -> act(BN_eval(BasicConv([x, max_k(src[idx] - x)])))
    as (B*N, 2C) bf16 (reference torch_vertex.py:47-62 + torch_nn.py:57-69)."""
    lib = _lib.load()
    B, N, C = x.shape
    M = N if src is None else src.shape[1]
    x = x.contiguous()
    src = None if src is None else src.contiguous()
    a, c = bn_passes.eval_ac(lib, bn, conv.bias, 2 * C)
    out = torch.empty((B * N, 2 * C), dtype=torch.bfloat16, device=x.device)
    fn = lib.gkg_mr_linear_bf16_nn16 if nn_idx.dtype == torch.int16 else lib.gkg_mr_linear_bf16      # compact lists: knn_graph_tm16
    _lib.check(fn(_ptr(x), _ptr(src), _ptr(nn_idx), _ptr(derived.mr_planes(conv)), _ptr(a), _ptr(c), _ptr(out),
                  2 * C, B, G, C // G, N, M, nn_idx.shape[2], act, _stream()), "gkg_mr_linear_bf16")
    return out


# ----------------------------------------------------------------------------------------------- block drivers
def _bn_ok(bn) -> bool:
    if not isinstance(bn, torch.nn.modules.batchnorm._BatchNorm) or not bn.affine or bn.momentum is None:
        return False
    return True                 # SyncBatchNorm across ranks: the statistics are all-reduced inside the fused path


def fused_supported(mod, x, groups: int) -> bool:
    """Fused path preconditions: fp32 CUDA input (any dtype under autocast), 'mr' aggregation with GELU+BN, channel
    counts that keep float4 / group boundaries aligned.  BatchNorm and SyncBatchNorm (statistics all-reduced inside the
    path) are both handled, each layer in train mode or in eval mode (frozen: running statistics, gkg_bn_eval_bwd in the
    backward) independently of the module's own mode."""
    from .graph import MRConv2d
    gc = mod.graph_conv
    C = mod.channels
    # fp32 activations; under autocast (mixed precision) bf16 inputs are accepted too: the block then keeps its
    # activations in fp32 and only the projection GEMMs run on bf16 operands (fp32 accumulation)
    if not x.is_cuda or not (x.dtype == _F32 or (x.dtype in (torch.bfloat16, torch.float16) and torch.is_autocast_enabled())):
        return False
    if not isinstance(gc.gconv, MRConv2d) or len(gc.gconv.nn) != 3 or not isinstance(gc.gconv.nn[2], torch.nn.GELU):
        return False
    if C % 16 or (C // groups) % 4 or getattr(gc.dilated_knn_graph, "stochastic", False):
        return False
    bns = [mod.fc1[1], gc.gconv.nn[1], mod.fc2[1]]
    if hasattr(mod, "ffn"):
        bns += [mod.ffn.fc1[1], mod.ffn.fc2[1]]
        if not isinstance(mod.ffn.act, torch.nn.GELU):
            return False
    if not all(_bn_ok(b) for b in bns):
        return False
    return ENABLED


def _train_16bit(x, conv, bn):
    """Which own 16-bit products _LinearBNAct takes for this layer, as (kind, conv) — the row of linear_bf16.KINDS whose switch is on
    (GKG_ENABLE=train_bf16 / train_f16) and whose predicate holds (linear_bf16.train16_ok: its autocast dtype among the rest), with the
    module its fragment arrays are cached on — or None.  Asked here, where the caller's gradient mode and autocast state are still
    visible.  The kinds exclude each other by the autocast dtype, so both switches may be on; bf16 is asked first."""
    for kind, on in ((BF16, TRAIN_BF16), (F16, TRAIN_F16)):
        if train16_ok(kind, on, x, conv, bn):
            return kind, conv
    return None


def _train_grouped_16bit(XM, conv, bn):
    """Which own GROUPED 16-bit products _GroupedLinearBNAct takes for this layer, as (kind, conv), or None: GKG_ENABLE=train_grouped
    acts only beside the kind's own switch (train_bf16 under bf16 autocast, train_f16 under fp16 autocast), and the predicate
    (linear_bf16.train16_grouped_ok) holds.  Asked by the callers (_graph_and_project, _aggregate_project), where the gradient mode
    and the autocast state are still visible.  GKG_DETERMINISTIC is not asked: these two products add nothing atomically."""
    if not TRAIN_GROUPED:
        return None
    for kind, on in ((BF16, TRAIN_BF16), (F16, TRAIN_F16)):
        if train16_grouped_ok(kind, on, XM, conv, bn):
            return kind, conv
    return None


def _lin(x, seq, act=0, residual=None, nchw=None, out_lowp=False, scale=None, rows_per_scale=0, want16=False, alias=False,
         dual=False, xm=None, knn=None, chain=False):
    """``scale`` (one factor per image; token-major outputs: per ``rows_per_scale`` consecutive rows) multiplies the BN
    output before the residual is added: the reference's DropPath on the branch (torch_vertex.py:332,355,402).
    ``alias``: returns ``(out, x')`` with ``x'`` the input again, to be used as a later layer's residual (see
    _LinearBNAct.forward).  ``chain``: the caller is a Grapher / FFN on the channels-last chain (what GKG_ENABLE=lin_bf16
    covers)."""
    if alias:
        if not (torch.is_grad_enabled() and x.requires_grad):
            return _lin(x, seq, act, residual, nchw, out_lowp, scale, rows_per_scale, want16, xm=xm, knn=knn), x
        conv, bn = seq[0], seq[1]
        w16 = derived.w16(conv) if x.dtype == torch.bfloat16 else None
        return _LinearBNAct.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, residual, bn, act, nchw, out_lowp, w16, scale,
                                  rows_per_scale, want16, True, False, xm, knn, _train_16bit(x, conv, bn))
    conv, bn = seq[0], seq[1]
    if knn is not None and lowp_inference():
        # only grapher_forward's bf16-inference branch hands a problem over here (both switches on): fc1 + the k-NN's token
        # preparation in one launch where the predicate takes it, else fc1 as without the problem
        if (not out_lowp and not want16 and act == 0 and residual is None
                and lin_bf16_prep_ok(LIN_BF16 and LIN_BF16_PREP, True, x, conv, bn, knn, chain, nchw, scale, xm, alias, dual)):
            return linear_bf16_knn_prep_eval(x, conv, bn, knn)
        knn = None
    if LIN_BF16 and lin_bf16_ok(LIN_BF16, lowp_inference(), x, conv, bn, chain, nchw, scale, xm, knn, alias, dual):
        # bf16 inference, opt-in: the library's own projection kernel, BN (+ GELU) (+ residual) and both precisions in its epilogue
        o32, o16 = linear_bf16_eval(x, conv, bn, act, residual, want_f32=not out_lowp, want_bf16=out_lowp or want16)
        if out_lowp:
            return o16
        if want16:
            o32._gkg_bf16_tm = o16
        return o32
    if (FOLD_EPILOGUE and out_lowp and x.dtype == torch.bfloat16 and residual is None and nchw is None and scale is None
            and not torch.is_grad_enabled() and not bn.training and bn.track_running_stats and conv.weight.dim() == 4
            and conv.groups == 1):
        # bf16 inference, activation only feeds the next GEMM: BN folded into the weights, bias (+ GELU) in the GEMM epilogue
        wf, cf, _ = derived.folded(conv, bn)
        return torch._addmm_activation(cf, x, wf.t(), use_gelu=(act == 1))
    if (FOLD_EPILOGUE and not out_lowp and act == 0 and x.dtype == torch.bfloat16 and residual is None and nchw is None
            and scale is None and not want16 and not torch.is_grad_enabled() and not bn.training and bn.track_running_stats
            and conv.weight.dim() == 4 and conv.groups == 1):
        # bf16 inference, fp32 result wanted (the Grapher's fc1: the k-NN and the aggregation read it in fp32): BN scale
        # folded into the bf16 weights, the shift as an fp32 bias in the GEMM epilogue, fp32 accumulate AND fp32 output
        wf, _, cf32 = derived.folded(conv, bn)
        return torch.addmm(cf32, x, wf.t(), out_dtype=_F32)
    w16 = derived.w16(conv) if x.dtype == torch.bfloat16 else None
    return _LinearBNAct.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, residual, bn, act, nchw, out_lowp, w16, scale,
                              rows_per_scale, want16, False, dual, xm, knn, _train_16bit(x, conv, bn))


# ---- a block output in both layouts (round 5) ---------------------------------------------------------------------------
# A Grapher that takes and returns NCHW (the drop-in case: reference torch_vertex.py:325-333) in front of a GrapherLabel, which
# reads the feature map token-major as keys / values (torch_vertex.py:392-403): the label branch paid nchw_to_tm in its forward
# and, in the backward, token-major gradient -> NCHW, autograd's add with the other gradient, -> token-major again (8 + 25 of
# 981 us at cfg2).  Instead the block's last kernel writes its result token-major as well (the residual read from the block's
# own token-major copy of the input), the label branch takes that companion (``features._gkg_tm``), and the node's backward
# sums the two upstream gradients while it re-lays out the NCHW one.  Adaptive: a GrapherLabel that has to convert a feature
# map marks the block that produced it (``_gkg_producer``), which emits the companion from its next call on — blocks nobody
# reads token-major never pay the second store.  GKG_DISABLE=dual_layout: off.
DUAL_LAYOUT = "dual_layout" not in _DISABLED


def _drop_scale(drop_path, batch, device):
    return drop_path.sample_scale(batch, device) if hasattr(drop_path, "sample_scale") else None


def _graph_and_project(x1b, yb, relative_pos, gc, groups, C, lp, want_edge):
    """DyGraphConv2d.forward on token-major tensors (torch_vertex.py:191-205): -> (BasicConv output (T, 2C), edge_index | None).
    ``x1b``: (B, N, C) or the x half of an XM operand buffer (see _xm_xview)."""
    nn_ = gc.gconv.nn
    N = x1b.shape[1]
    if _knn_mr_ok(x1b, yb, relative_pos, gc.k, gc.d, groups, nn_, lp):      # row g2: graph + aggregation in one kernel
        XM, edge = _KnnMaxRelativeTM.apply(x1b, yb, relative_pos, gc.k, gc.d, groups, want_edge)
        a2 = _GroupedLinearBNAct.apply(XM, nn_[0].weight, nn_[0].bias, nn_[1].weight, nn_[1].bias, nn_[1], 1, False, None,
                                       _train_grouped_16bit(XM, nn_[0], nn_[1]))
        return a2, (edge if want_edge else None)
    nn_idx, edge = _graph_lists(x1b, yb, relative_pos, gc, groups, want_edge)
    return _aggregate_project(x1b, yb, nn_idx, groups, nn_, C, lp), edge       # row g1: aggregation = the projection's operand producer


def _graph_lists(x1b, yb, relative_pos, gc, groups, want_edge):
    """The k-NN call of a block whose graph and aggregation are separate launches -> (neighbour lists (B G, N, k), edge_index | None):
    the compact u16 lists where nobody asked for the graph, else the int64 edge_index and its neighbour plane."""
    M = x1b.shape[1] if yb is None else yb.shape[1]
    if KNN_COMPACT and not want_edge and M <= 65536 and knn_graph_tm is _KNN_GRAPH_TM:
        return knn_graph_tm16(x1b, yb, relative_pos, gc.k, gc.d, groups), None  # u16 lists: no int64 edge_index, no centre plane
    edge = knn_graph_tm(x1b, yb, relative_pos, gc.k, gc.d, groups)
    return edge[0], edge


# fc1's output written straight into the grouped projection's operand buffer (see _LinearBNAct.forward ``xm``): fp32 blocks
# outside the bf16-inference form (whose fused kernel never materialises the operand).  False: fc1 writes a plain (T, C) matrix
# and the aggregation copies x into the buffer next to m — a module constant for the A/B tests, no environment switch.
XM_DIRECT = True
# fc1's BN-apply pass is also the k-NN's token preparation (gkg_bn_apply_knn_prep; needs XM_DIRECT).  A module constant for the
# A/B tests (identical bits either way), no environment switch.
KNN_PREP = True


def grapher_forward(mod, x, relative_pos, groups: int, want_edge: bool = True):
    """Fused Grapher.forward (reference torch_vertex.py:325-333).  Returns (out (B,C,H,W), edge_index); ``want_edge=False``
    (Grapher.forward, which discards the graph like the reference, torch_vertex.py:330): edge_index may be None."""
    B, C, H, W = x.shape
    N = H * W
    gc = mod.graph_conv
    lp = lowp_inference()
    if not lp:
        from . import block
        want_tm = DUAL_LAYOUT and getattr(mod, "_gkg_want_tm", False)
        if block.grapher_ok(mod, x, relative_pos, groups, want_edge, want_tm):
            # the whole block as ONE library call per direction (block.py / csrc/gkg_block.hip): same launches, same bits
            return block.grapher_forward(mod, x, relative_pos, groups, want_tm), None      # (companion / producer marks set there)
    xt, x, cl = _block_entry(x, lp)                                 # (T, C) and the residual branch
    scale = _drop_scale(mod.drop_path, B, x.device)
    dual = (DUAL_LAYOUT and not cl and not lp and scale is None and torch.is_grad_enabled() and xt.dtype == _F32
            and getattr(mod, "_gkg_want_tm", False))
    xm = (B, N) if (XM_DIRECT and not lp and xt.dtype == _F32 and not torch.is_autocast_enabled() and C % 16 == 0) else None
    # fc1's BN-apply also prepares the k-NN's queries (normalised copies, norms): no token-preparation launch behind it
    Mk = (H // gc.r) * (W // gc.r) if gc.r > 1 else N
    knn = _knn_key_for(B, N, C, Mk, gc.r > 1, relative_pos, gc, groups, lp, want_edge) if (xm is not None and KNN_PREP) else None
    if lp and cl and LIN_BF16 and LIN_BF16_PREP and KNN_PREP:
        # bf16 inference on the channels-last chain: the own projection kernel prepares the queries in fc1's launch (pooled keys,
        # r > 1, are prepared by the k-NN call as always)
        knn = _knn_key_for(B, N, C, Mk, gc.r > 1, relative_pos, gc, groups, lp, want_edge, lp_prep=True)
    if dual:
        x1, xt_r = _lin(xt, mod.fc1, alias=True, xm=xm, knn=knn)    # xt_r: xt again, the (token-major) residual of fc2
    else:
        x1 = _lin(xt, mod.fc1, xm=xm, knn=knn, chain=cl)            # fc1 + BN
    x1b = x1 if xm is not None else x1.view(B, N, C)
    if xm is None and getattr(x1, "_gkg_knn", None) is not None:
        x1._gkg_knn.mark(x1b)                                       # the view is a new object: the mark travels with the tokens
    yb = None
    if gc.r > 1:                                                    # pooled keys (torch_vertex.py:194-196)
        yb = _AvgPoolTM.apply(x1b, H, W, gc.r)
    if cl and lp and LIN_BF16 and MR_FC2_BF16:
        # bf16 inference on the channels-last chain, opt-in: the graph, then aggregation + grouped projection + fc2 in ONE launch where
        # the predicate takes it (the (T, 2C) matrix stays on chip: the pair's bits), else the two launches as below
        nn_idx, edge = _graph_lists(x1b, yb, relative_pos, gc, groups, want_edge)
        if mr_fc2_bf16_ok(MR_FC2_BF16, lp, x1b, yb, nn_idx, groups, gc.gconv.nn, mod.fc2, x, scale, True):
            out, o16 = mr_fc2_bf16_eval(x1b, yb, nn_idx, groups, gc.gconv.nn, mod.fc2, x, want_f32=True, want_bf16=True)
            out._gkg_bf16_tm = o16
        else:
            a2 = _aggregate_project(x1b, yb, nn_idx, groups, gc.gconv.nn, C, lp)
            out = _lin(a2, mod.fc2, residual=x, scale=scale, rows_per_scale=N, want16=lp, chain=True)
        return _cl_out(out, B, H, W), edge
    a2, edge = _graph_and_project(x1b, yb, relative_pos, gc, groups, C, lp, want_edge)
    if cl:                                                          # fc2 + BN (+ DropPath) + residual, token-major = channels-last
        out = _lin(a2, mod.fc2, residual=x, scale=scale, rows_per_scale=N, want16=lp, chain=True)
        return _cl_out(out, B, H, W), edge
    if dual:
        # ... and, once the label block behind has said which k-NN problem it solves over this map (KnnProblem.announce), the same pass
        # prepares that problem's KEYS (gkg_bn_apply_knn_prep as_keys): the label graph launches no token preparation at all
        # (its workspace is allocated by the pass itself, only if it runs as the producer: KnnProblem.producer_args)
        kk = knn_prep.KnnProblem.keys_for_label(B, C, N, knn_prep.announced(mod)) if (KNN_PREP and _knn_ahead_ok()) else None
        out, out_tm = _lin(a2, mod.fc2, residual=xt_r, nchw=(B, C, H, W), dual=True, knn=kk)
        out._gkg_tm = (out._version, out_tm)                        # the token-major companion (grapher_label_forward)
        out._gkg_producer = weakref.ref(mod)
        return out, edge
    out = _lin(a2, mod.fc2, residual=x, nchw=(B, C, H, W), scale=scale)      # ... back to NCHW
    if DUAL_LAYOUT:
        out._gkg_producer = weakref.ref(mod)
    return out, edge


def _label_features(features, B, C):
    """The feature map as a GrapherLabel reads it -> (keys / values token-major (B, HW, C), contiguous; the prepared-keys object the
    producing block left on its token-major companion | None; the producing module | None)."""
    ent = getattr(features, "_gkg_tm", None)
    keys_key = None
    prod = getattr(features, "_gkg_producer", None)
    prod = prod() if prod is not None else None
    if is_channels_last(features):                                           # keys / values (B, HW, C): a view
        ft = features.permute(0, 2, 3, 1).reshape(B, -1, C)
    elif (DUAL_LAYOUT and ent is not None and ent[0] == features._version and features.dim() == 4 and features.dtype == _F32
          and ent[1].shape == (B * features.shape[2] * features.shape[3], C)):
        ft = ent[1].view(B, -1, C)                                           # the producing block's token-major companion
        keys_key = knn_prep.prepared_keys(ent[1])                            # ... which may carry this graph's prepared keys
    else:
        if prod is not None and not prod.__dict__.get("_gkg_want_tm", False):
            prod._gkg_want_tm = True                                         # ... which it emits from its next call on
        ft = to_token_major(features.float().contiguous()).view(B, -1, C)
    return ft.contiguous(), keys_key, prod


def grapher_label_forward(mod, e, features, groups: int):
    """Fused GrapherLabel.forward (reference torch_vertex.py:392-403).  Returns (E' (B,L,C), edge_index (2,BG,L,k))."""
    B, L, C = e.shape
    gc = mod.graph_conv
    ftc, keys_key, prod = _label_features(features, B, C)
    e2 = e.float().reshape(B * L, C).contiguous()
    lp = lowp_inference()
    xm = (B, L) if (XM_DIRECT and not lp and not torch.is_autocast_enabled() and C % 16 == 0) else None
    knn = _knn_key_for(B, L, C, ftc.shape[1], True, None, gc, groups, lp, True) if (xm is not None and KNN_PREP) else None
    if knn is not None:
        knn.adopt_keys(keys_key)                 # the producing Grapher prepared the keys: its workspace is this call's
        knn.announce(prod, groups, L)            # ... or it does, from its next call on
    if not lp:
        from . import block
        if block.label_ok(mod, e, ftc, groups):
            out, edge = block.label_forward(mod, e2, ftc, groups, keys_key)          # ONE library call per direction (block.py)
            return out.view(B, L, C), edge
    x1, e2r = _lin(e2, mod.fc1, alias=True, xm=xm, knn=knn)          # e2r: e2 again, for the residual of fc2 (one gradient node)
    x1b = x1 if xm is not None else x1.view(B, L, C)
    a2, edge = _graph_and_project(x1b, ftc, None, gc, groups, C, lp, True)      # GrapherLabel returns its graph
    h2 = _lin(a2, mod.fc2, residual=e2r, scale=_drop_scale(mod.drop_path, B, e.device), rows_per_scale=L)
    f1, h2r = _lin(h2, mod.ffn.fc1, act=1, out_lowp=lp, alias=True)
    out = _lin(f1, mod.ffn.fc2, residual=h2r, scale=_drop_scale(mod.ffn.drop_path, B, e.device), rows_per_scale=L)
    return out.view(B, L, C), edge


def ffn_supported(mod, x) -> bool:
    """Fused path for the backbone's FFN block (1x1 conv + BN + GELU -> 1x1 conv + BN -> + residual)."""
    if not (ENABLED and x.is_cuda and x.dim() == 4):
        return False
    if not (x.dtype == _F32 or (x.dtype in (torch.bfloat16, torch.float16) and torch.is_autocast_enabled())):
        return False
    if not isinstance(mod.act, torch.nn.GELU) or not (_bn_ok(mod.fc1[1]) and _bn_ok(mod.fc2[1])):
        return False
    if any(conv.weight.shape[0] % 4 or conv.weight.shape[1] % 4 for conv in (mod.fc1[0], mod.fc2[0])):
        return False
    return True


def ffn_forward(mod, x):
    """reference gkgnet.py:66-72 on token-major activations: two library GEMMs + the BN/GELU/residual kernels (bf16 inference,
    opt-in: the two projections on the own bf16 kernel, as two launches or — GKG_ENABLE=lin_bf16,ffn_bf16 — as one)."""
    lp = lowp_inference()
    B, C, H, W = x.shape
    xt, x, cl = _block_entry(x, lp)
    if cl:
        scale = _drop_scale(mod.drop_path, B, x.device)
        if LIN_BF16 and ffn_bf16_ok(FFN_BF16, lp, xt, mod.fc1, mod.fc2, x, scale, True):
            # bf16 inference, opt-in: both projections in ONE launch, the (T, 4C) hidden matrix stays on chip (the pair's bits)
            out, o16 = ffn_bf16_eval(xt, mod.fc1, mod.fc2, x, want_f32=True, want_bf16=True)
            out._gkg_bf16_tm = o16
        else:
            h = _lin(xt, mod.fc1, act=1, out_lowp=lp, chain=True)
            out = _lin(h, mod.fc2, residual=x, scale=scale, rows_per_scale=H * W, want16=lp, chain=True)
        return _cl_out(out, B, H, W)
    h = _lin(xt, mod.fc1, act=1, out_lowp=lp)
    return _lin(h, mod.fc2, residual=x, nchw=(B, C, H, W), scale=_drop_scale(mod.drop_path, B, x.device))
