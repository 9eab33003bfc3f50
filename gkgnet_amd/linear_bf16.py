"""bf16 inference: a dense 1x1 projection with its eval-mode BN (+ GELU) (+ residual) as ONE launch of the library's own kernel
(gkg_linear_bf16, csrc/gkg_linear_bf16.hip) — the call (the weight's fragment array: derived.lin_planes) and the predicate ``fused._lin`` asks before
it dispatches here — and the same launch with the k-NN's token preparation riding on it (gkg_linear_bf16_knn_prep: a Grapher's
fc1) — and an FFN's two projections as one launch with the hidden matrix kept on chip (gkg_ffn_bf16, csrc/gkg_ffn_bf16.hip) — and a Grapher's aggregation, grouped projection and fc2 as one launch
(gkg_mr_fc2_bf16, csrc/gkg_mr_fc2_bf16.hip).  Also the training side (GKG_ENABLE=train_bf16 / train_f16): the same kernel reading an fp32 A
operand for a layer's forward and input gradient, in bf16 (gkg_linear_bf16_f32a) or IEEE fp16 (gkg_linear_f16_f32a).  What differs
between the two element kinds is one row each of ``KINDS`` (autocast dtype, entry-point names, fragment dtype, derived's two slots,
``own_wgrad``); the predicate and the two products (train16_ok, train16_fwd, train16_dgrad) are written once against it, and the bf16
weight-gradient kernel (gkg_linear_wgrad_bf16, linear_bf16_wgrad) is the one thing only bf16 has.  With GKG_ENABLE=train_grouped beside
either switch the GROUPED projection between a Grapher's dense layers takes its forward and input gradient from the kernel's grouped
form, again written once against the row (train16_grouped_ok, train16_grouped_fwd, train16_grouped_dgrad).  Mechanism only: the
switches (``fused.LIN_BF16``, ``fused.LIN_BF16_PREP``, ``fused.FFN_BF16``, ``fused.MR_FC2_BF16``, ``fused.TRAIN_BF16``, ``fused.TRAIN_F16``, ``fused.TRAIN_GROUPED``) and the mode test (``fused.lowp_inference``) stay in
``fused.py`` and arrive as arguments."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib, bn_passes, derived
from .ops import _ptr, _stream

_F32 = torch.float32


def lin_bf16_ok(on, lp, x, conv, bn, chain=True, nchw=None, scale=None, xm=None, knn=None, alias=False, dual=False,
                supported=None) -> bool:
    """Whether ``fused._lin`` hands this layer to linear_bf16_eval.  ``on``: the opt-in switch; ``lp``: bf16 autocast with gradients
    off; ``chain``: the caller is on the channels-last chain (its operand and residual are token-major views).  Reads only
    ``x.dtype`` / ``x.shape``, ``conv.groups`` / ``conv.weight.shape`` and ``bn.training`` / ``bn.track_running_stats``;
    ``supported(R, cin, cout)`` stands in for the library's own answer (tests)."""
    if not (on and lp and chain) or x.dtype != torch.bfloat16:
        return False
    if nchw is not None or scale is not None or xm is not None or knn is not None or alias or dual:
        return False
    if bn.training or not bn.track_running_stats or conv.groups != 1:
        return False
    wshape = tuple(conv.weight.shape)
    if len(x.shape) != 2 or len(wshape) != 4 or wshape[2:] != (1, 1) or wshape[1] != x.shape[1]:
        return False
    if supported is None:
        return bool(_lib.load().gkg_linear_bf16_supported(x.shape[0], wshape[1], wshape[0], 0, 1, 0, 0))
    return bool(supported(x.shape[0], wshape[1], wshape[0]))


def _rows(t, align):
    """A 2-d tensor as the kernel addresses it: unit column stride, row pitch a multiple of ``align`` elements, 16-byte base."""
    if t.stride(1) != 1 or t.stride(0) % align or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        t = t.contiguous()
    return t


@torch.no_grad()
def linear_bf16_eval(x16, conv, bn, act=0, residual=None, want_f32=True, want_bf16=False):
    """x16 (R, cin) bf16 -> act(BN_eval(Conv1x1(x16))) (+ residual (R, cout) fp32) as (out_f32 | None, out_bf16 | None), each
    (R, cout) (reference torch_vertex.py:290-306, gkgnet.py:46-72).  The BN scale stays an fp32 vector of the epilogue: the bf16
    weight is the parameter's own rounding, not a folded copy."""
    lib = _lib.load()
    R, cin = x16.shape
    cout = conv.weight.shape[0]
    assert x16.dtype == torch.bfloat16 and (want_f32 or want_bf16)
    x16 = _rows(x16, 8)
    if residual is not None:
        assert residual.dtype == _F32 and tuple(residual.shape) == (R, cout)
        residual = _rows(residual, 4)
    a, c = bn_passes.eval_ac(lib, bn, conv.bias, cout)
    o32 = torch.empty((R, cout), dtype=_F32, device=x16.device) if want_f32 else None
    o16 = torch.empty((R, cout), dtype=torch.bfloat16, device=x16.device) if want_bf16 else None
    _lib.check(lib.gkg_linear_bf16(_ptr(x16), x16.stride(0), _ptr(derived.lin_planes(conv)), _ptr(a), _ptr(c), _ptr(residual),
                                   0 if residual is None else residual.stride(0), _ptr(o32), cout, _ptr(o16), cout, R, cin, cout,
                                   act, _stream()), "gkg_linear_bf16")
    return o32, o16


# ---- an FFN as one launch (gkg_ffn_bf16, csrc/gkg_ffn_bf16.hip): fc1 + BN + GELU + fc2 + BN + residual, the hidden kept on chip ----
# No dispatch rule beyond the library's envelope (cin, cout <= 192): every FFN shape inside it measured faster than the pair of
# gkg_linear_bf16 launches.  MI355X, tools/bench_lin_bf16.py --ffn, us per FFN, median of 11 alternating replays [min, max], one box
# (EXPERIMENTS.md "Fused bf16 FFN", profiles/ffn_bf16_layers_*.txt):
#   cfg3 (GKGNet-576, B 32)   C  80  hid 320  R 663 552   pair 543 [534, 581]   fused 296 [285, 317]
#                             C 160  hid 640  R 165 888   pair 337 [333, 342]   fused 234 [231, 239]
#   cfg5 (pvig_m 768^2, B 16) C  96  hid 384  R 589 824   pair 535 [516, 570]   fused 314 [309, 338]
#                             C 192  hid 768  R 147 456   pair 344 [338, 350]   fused 244 [240, 251]
# (C 400 / 640 / 384 / 768, stages 3-4: outside the envelope, the two launches.)
class _Rows:
    """What lin_bf16_ok reads of an operand (dtype, shape): the bf16 hidden matrix the fused launch never makes."""

    def __init__(self, R, C):
        self.dtype, self.shape = torch.bfloat16, (R, C)


def ffn_bf16_ok(on, lp, x, fc1, fc2, residual, scale, chain, supported=None, act=1) -> bool:
    """Whether ``fused.ffn_forward`` hands the FFN (``fc1`` / ``fc2``: its (conv, bn) pairs) to ffn_bf16_eval instead of two
    linear_bf16_eval calls: the switch, lin_bf16_ok for both layers (bf16 autocast with gradients off, the channels-last chain,
    eval-mode BN, dense 1x1 convs), no DropPath scale, a GELU on the hidden (``act`` == 1), an fp32 residual of the output's shape
    (or none) and the library's answer for the sizes (``supported(R, cin, hid, cout)`` stands in for it in tests)."""
    if not on or scale is not None or act != 1:
        return False
    fine = (lambda R, ci, co: True) if supported is not None else None        # the pair's own answer is asked below, once
    if not lin_bf16_ok(on, lp, x, fc1[0], fc1[1], chain, scale=scale, supported=fine):
        return False
    R, cin, hid = x.shape[0], x.shape[1], fc1[0].weight.shape[0]
    if not lin_bf16_ok(on, lp, _Rows(R, hid), fc2[0], fc2[1], chain, scale=scale, supported=fine):
        return False
    cout = fc2[0].weight.shape[0]
    if residual is not None and (residual.dtype != _F32 or tuple(residual.shape) != (R, cout)):
        return False
    if supported is not None:
        return bool(supported(R, cin, hid, cout))
    return bool(_lib.load().gkg_ffn_bf16_supported(R, cin, hid, cout, int(residual is not None), 1, 1, 1))


@torch.no_grad()
def ffn_bf16_eval(x16, fc1, fc2, residual=None, want_f32=True, want_bf16=False):
    """x16 (R, cin) bf16 -> BN2(fc2(bf16(GELU(BN1(fc1(x16)))))) (+ residual (R, cout) fp32) as (out_f32 | None, out_bf16 | None): the
    bits of linear_bf16_eval(x16, *fc1, act=1, want_f32=False, want_bf16=True) followed by linear_bf16_eval(h16, *fc2, 0, residual,
    ...), in one launch that keeps the (R, hid) hidden matrix on chip (reference gkgnet.py:66-72)."""
    lib = _lib.load()
    R, cin = x16.shape
    (conv1, bn1), (conv2, bn2) = (fc1[0], fc1[1]), (fc2[0], fc2[1])
    hid, cout = conv1.weight.shape[0], conv2.weight.shape[0]
    assert x16.dtype == torch.bfloat16 and conv2.weight.shape[1] == hid and (want_f32 or want_bf16)
    x16 = _rows(x16, 8)
    if residual is not None:
        assert residual.dtype == _F32 and tuple(residual.shape) == (R, cout)
        residual = _rows(residual, 4)
    a1, c1 = bn_passes.eval_ac(lib, bn1, conv1.bias, hid)
    a2, c2 = bn_passes.eval_ac(lib, bn2, conv2.bias, cout)
    o32 = torch.empty((R, cout), dtype=_F32, device=x16.device) if want_f32 else None
    o16 = torch.empty((R, cout), dtype=torch.bfloat16, device=x16.device) if want_bf16 else None
    _lib.check(lib.gkg_ffn_bf16(_ptr(x16), x16.stride(0), _ptr(derived.lin_planes(conv1)), _ptr(a1), _ptr(c1),
                                _ptr(derived.lin_planes(conv2)), _ptr(a2), _ptr(c2), _ptr(residual),
                                0 if residual is None else residual.stride(0), _ptr(o32), cout, _ptr(o16), cout, R, cin, hid, cout,
                                1, _stream()), "gkg_ffn_bf16")
    return o32, o16


# ---- a Grapher's tail as one launch (gkg_mr_fc2_bf16, csrc/gkg_mr_fc2_bf16.hip): aggregation + grouped projection + BN + GELU + fc2 +
# BN + residual, the (T, 2C) bf16 matrix between the two projections kept on chip ---------------------------------------------------
# DISPATCH RULE (``mr_fc2_pays``): the fused launch only where it measured at least as fast as the pair it replaces
# (gkg_mr_linear_bf16_nn16 -> gkg_linear_bf16) beyond the spread of the repeated pair measurements.
# MI355X, tools/bench_lin_bf16.py --tail, us per Grapher tail over the lists gkg_knn_fwd_tm16 finds for seeded tokens, median of 11
# alternating replays [min, max], two runs per config on one box (EXPERIMENTS.md "Fused bf16 Grapher tail",
# profiles/mr_fc2_bf16_layers_*.txt):
#   cfg3 (GKGNet-576, B 32)   C  80  G 2  k  9  R 663 552   pair 533 [524, 552] / 531   fused 430 [420, 445] / 427   taken
#                             C 160  G 2  k  9  R 165 888   pair 324 [322, 326] / 328   fused 245 [242, 247] / 247   taken
#   cfg5 (pvig_m 768^2, B 16) C  96  G 8  k 18  R 589 824   pair 986 [975, 1031] / 994  fused 909 [901, 944] / 915   taken
#                             C 192  G 8  k 18  R 147 456   pair 454 [448, 460] / 451   fused 380 [379, 381] / 378   taken
# (C 400 / 640 / 384 / 768, stages 3-4: outside the library's envelope, the two launches.)
# Every measured class is faster than the pair by more than the pair's two medians differ (2-9 us): the rule keeps all four.  The
# narrowest margin is cfg5 stage 1 (1.08x: k = 18 keeps the gather at two workgroups per CU); nothing was measured below these row
# counts, so the rule takes the measured widths' envelope and says nothing about size:
MR_FC2_MAX_C = 192


def mr_fc2_pays(T, C) -> bool:
    """The measured dispatch rule above: rows and channels of a Grapher."""
    return C <= MR_FC2_MAX_C


def mr_fc2_bf16_ok(on, lp, x, src, nn_idx, G, nn_, fc2, residual, scale, chain, supported=None) -> bool:
    """Whether ``fused.grapher_forward`` hands the second half of a Grapher — the aggregation over ``nn_idx`` (B G, N, k) of ``x``
    (B, N, C) fp32 (keys ``src`` (B, M, C) | None), the grouped projection ``nn_`` (conv, bn, GELU) and ``fc2`` (conv, bn) — to
    mr_fc2_bf16_eval instead of mr_grouped_linear_eval + linear_bf16_eval: the switch (``on`` == "all" —
    GKG_ENABLE=mr_fc2_bf16_all, tests, measurements — skips the measured rule: every shape the library takes), the conditions of the
    first launch (``fused._mr_gemm_ok``: bf16 autocast with gradients off, eval-mode BN, groups == 4, ``fused.MR_GEMM``; c % 4 == 0),
    lin_bf16_ok for fc2 on the (T, 2C) bf16 matrix the launch never makes (the channels-last chain, eval-mode BN, a dense 1x1 conv), no
    DropPath scale, an fp32 residual of the output's shape (or none) and the library's answer for the sizes
    (``supported(B, G, c, N, M, k)`` stands in for it in tests)."""
    if not on or scale is not None or len(x.shape) != 3 or x.dtype != _F32:
        return False
    from . import fused
    B, N, C = x.shape
    if G <= 0 or C % G or (C // G) % 4 or not fused._mr_gemm_ok(nn_, C, lp):
        return False
    if src is not None and (src.dtype != _F32 or len(src.shape) != 3 or src.shape[0] != B or src.shape[2] != C):
        return False
    M = N if src is None else src.shape[1]
    if len(nn_idx.shape) != 3 or tuple(nn_idx.shape[:2]) != (B * G, N) or (nn_idx.dtype == torch.int16 and M > 65536):
        return False
    fine = (lambda R, ci, co: True) if supported is not None else None        # the pair's own answer is asked below, once
    if not lin_bf16_ok(on, lp, _Rows(B * N, 2 * C), fc2[0], fc2[1], chain, scale=scale, supported=fine):
        return False
    if fc2[0].weight.shape[0] != C:
        return False
    if residual is not None and (residual.dtype != _F32 or tuple(residual.shape) != (B * N, C)):
        return False
    if on != "all" and not mr_fc2_pays(B * N, C):
        return False
    k = nn_idx.shape[2]
    if supported is not None:
        return bool(supported(B, G, C // G, N, M, k))
    return bool(_lib.load().gkg_mr_fc2_bf16_supported(B, G, C // G, N, M, k, int(residual is not None), 1, 1, 1))


@torch.no_grad()
def mr_fc2_bf16_eval(x, src, nn_idx, G, nn_, fc2, residual=None, want_f32=True, want_bf16=False):
    """x (B, N, C) fp32, src (B, M, C) fp32 | None, nn_idx (B G, N, k) int64 | int16 (the bits of u16 rows) ->
    BN2(fc2(bf16(GELU(BN1(BasicConv([x, max_k(src[idx] - x)])))))) (+ residual (B N, C) fp32) as (out_f32 | None, out_bf16 | None): the
    bits of fused.mr_grouped_linear_eval(x, src, nn_idx, G, *nn_) followed by linear_bf16_eval(h16, *fc2, 0, residual, ...), in one
    launch that keeps the (B N, 2C) matrix on chip (reference torch_vertex.py:47-62, torch_nn.py:57-69, torch_vertex.py:325-333)."""
    lib = _lib.load()
    B, N, C = x.shape
    M = N if src is None else src.shape[1]
    (conv1, bn1), (conv2, bn2) = (nn_[0], nn_[1]), (fc2[0], fc2[1])
    assert x.dtype == _F32 and conv2.weight.shape[1] == 2 * C and conv2.weight.shape[0] == C and (want_f32 or want_bf16)
    x = x.contiguous()
    src = None if src is None else src.contiguous()
    nn_idx = nn_idx.contiguous()
    if residual is not None:
        assert residual.dtype == _F32 and tuple(residual.shape) == (B * N, C)
        residual = _rows(residual, 4)
    a1, c1 = bn_passes.eval_ac(lib, bn1, conv1.bias, 2 * C)
    a2, c2 = bn_passes.eval_ac(lib, bn2, conv2.bias, C)
    o32 = torch.empty((B * N, C), dtype=_F32, device=x.device) if want_f32 else None
    o16 = torch.empty((B * N, C), dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    fn = lib.gkg_mr_fc2_bf16_nn16 if nn_idx.dtype == torch.int16 else lib.gkg_mr_fc2_bf16      # compact lists: knn_graph_tm16
    _lib.check(fn(_ptr(x), _ptr(src), _ptr(nn_idx), _ptr(derived.mr_planes(conv1)), _ptr(a1), _ptr(c1),
                  _ptr(derived.lin_planes(conv2)), _ptr(a2), _ptr(c2), _ptr(residual), 0 if residual is None else residual.stride(0),
                  _ptr(o32), C, _ptr(o16), C, B, G, C // G, N, M, nn_idx.shape[2], 1, _stream()), "gkg_mr_fc2_bf16")
    return o32, o16


# ---- fc1 + the k-NN's token preparation in one launch (gkg_linear_bf16_knn_prep) ---------------------------------------------
# DISPATCH RULE (``prep_pays``): the fused launch only where it measured at least as fast as the pair it replaces (gkg_linear_bf16
# + the token_prep launch of the k-NN call), i.e. within the spread of the repeated pair measurements or better.  MI355X,
# tools/bench_lin_bf16.py --prep, us per (fc1 [+ prep] launch, k-NN call) pair, median of 11 alternating replays [min, max], two
# runs of cfg3 on one box (EXPERIMENTS.md, profiles/lin_bf16_prep_layers_*.txt):
#   cfg3 (GKGNet-576, B 32)   C  80  c  40  R 663 552   pair 1771 [1761, 1913] / 1769   fused 1751 [1743, 1887] / 1757   taken
#                             C 160  c  80  R 165 888   pair  776 [773, 781]            fused  908 [906, 916]            not taken
#                             C 400  c 200  R  41 472   pair  479 [477, 485]            fused  675 [626, 679]            not taken
#                             C 640  c 320  R  10 368   pair  150 [147, 151]            fused  252 [249, 254]            not taken
#   cfg5 (pvig_m 768^2, B 16) C  96  c  12  R 589 824   pair 6597 [6580, 6638]          fused 6580 [6552, 6625]          taken
#                             C 192  c  24  R 147 456   pair 2702 [2684, 2743]          fused 2745 [2732, 2758]          not taken
#                             C 384  c  48  R  36 864   pair  963 [958, 976]            fused 1008 [998, 1021]           not taken
#                             C 768  c  96  R   9 216   pair  220 [217, 223]            fused  303 [299, 306]            not taken
# The two winners are the stage-1 shapes: one 128-column tile holds every group, so each workgroup prepares the rows it has just
# stored (no hand-off between workgroups), with one thread per (row, group) pair (c <= 52).  Everywhere else the last arrival of
# a row tile runs the preparation of 128 rows x G groups behind its neighbours, and that serial tail costs more than the launch
# it removes — the wide 18 x 18 stages most (fc1 35 -> 159 us against a 22 us preparation launch).  The rule takes the measured
# winners and what lies beyond them in the direction the measurements support (more rows of the same form), nothing in between:
PREP_MAX_COUT, PREP_MAX_GROUP, PREP_MIN_ROWS = 128, 40, 1 << 19


def prep_pays(R, cout, c) -> bool:
    """The measured dispatch rule above: rows, columns and group width of a Grapher's fc1."""
    return cout <= PREP_MAX_COUT and c <= PREP_MAX_GROUP and R >= PREP_MIN_ROWS


def lin_bf16_prep_ok(on, lp, x, conv, bn, knn, chain=True, nchw=None, scale=None, xm=None, alias=False, dual=False,
                     supported=None, prep_supported=None) -> bool:
    """Whether ``fused._lin`` hands a Grapher's fc1 WITH its k-NN problem ``knn`` (a knn_prep.KnnProblem: queries, fp32 contraction)
    to linear_bf16_knn_prep_eval: lin_bf16_ok's conditions without its ``knn`` exclusion, a problem over exactly this layer's
    rows and columns, the measured rule (``on`` == "all" — GKG_ENABLE=lin_bf16_prep_all, tests, measurements — skips it: every
    shape the library takes) and the library's own answer (``prep_supported(cin, knn)`` stands in for it in tests)."""
    if knn is None or not lin_bf16_ok(on, lp, x, conv, bn, chain, nchw, scale, xm, None, alias, dual, supported):
        return False
    cout, cin = conv.weight.shape[0], conv.weight.shape[1]
    if knn.as_keys or knn.B * knn.N != x.shape[0] or knn.G * knn.c != cout or knn.c % 4:
        return False
    if on != "all" and not prep_pays(x.shape[0], cout, knn.c):
        return False
    if prep_supported is not None:
        return bool(prep_supported(cin, knn))
    return bool(_lib.load().gkg_linear_bf16_knn_prep_supported(cin, knn.B, knn.G, knn.c, knn.N, knn.M, knn.k, knn.d, knn.has_y,
                                                               knn.has_rp, knn.flags, knn.fused_mr))


_PREP_SCRATCH = {}       # (device, stream) -> the zeroed arrival counters every launch leaves zero (grown on demand)


def _prep_scratch(lib, device, stream, R) -> torch.Tensor:
    need = int(lib.gkg_linear_bf16_knn_prep_scratch_bytes(R))
    t = _PREP_SCRATCH.get((device, stream))
    if t is None or t.numel() < need:
        t = torch.zeros(max(need, 4096), dtype=torch.uint8, device=device)
        _PREP_SCRATCH[(device, stream)] = t
    return t


@torch.no_grad()
def linear_bf16_knn_prep_eval(x16, conv, bn, knn):
    """x16 (B N, cin) bf16 -> BN_eval(Conv1x1(x16)) (B N, G c) fp32 — the bits of linear_bf16_eval(x16, conv, bn)[0] — with the
    tokens prepared in ``knn``'s workspace as the queries of the k-NN call behind (reference torch_vertex.py:326 ->
    torch_edge.py:167-173); the result carries the problem (knn.mark)."""
    lib = _lib.load()
    R, cin = x16.shape
    cout = conv.weight.shape[0]
    assert x16.dtype == torch.bfloat16 and R == knn.B * knn.N and cout == knn.G * knn.c and not knn.as_keys
    x16 = _rows(x16, 8)
    a, c = bn_passes.eval_ac(lib, bn, conv.bias, cout)
    out = torch.empty((R, cout), dtype=_F32, device=x16.device)
    stream = _stream()
    scratch = _prep_scratch(lib, x16.device, stream, R)
    _lib.check(lib.gkg_linear_bf16_knn_prep(_ptr(x16), x16.stride(0), _ptr(derived.lin_planes(conv)), cin, _ptr(a), _ptr(c),
                                            *knn.producer_args(lib, out, None, None, cout, 0), _ptr(scratch), scratch.numel(),
                                            stream), "gkg_linear_bf16_knn_prep")
    knn.mark(out)
    return out


# ---- training under 16-bit autocast (GKG_ENABLE=train_bf16 / train_f16): a dense layer's products on the own kernel of that kind ----
# Y = x W^T and dx = dY W (+ the skip gradient) are the kind's ``*_f32a`` entry point: the projection kernel reading fp32 operands and
# rounding them on their way into LDS (bf16; or IEEE fp16, subnormals kept: a loss-scaled gradient's small values survive), fp32
# accumulation, no vendor GEMM, no cast launch.  What differs between the two kinds is a row of KINDS; everything below is written
# once against it.  bf16 alone has a weight-gradient kernel of its own (dW = dY^T x, gkg_linear_wgrad_bf16,
# csrc/gkg_linear_bf16_train.hip: atomically added slabs, hence refused under GKG_DETERMINISTIC); fp16's weight gradient stays where
# ``fused._wgrad`` puts it (the x6 kernels measured faster than a one-product 16-bit weight gradient at every cfg4 shape), so that kind
# adds nothing atomically and holds under GKG_DETERMINISTIC as well.  Mechanism only: ``fused.TRAIN_BF16`` / ``fused.TRAIN_F16``
# arrive as ``on``.
class Kind16(NamedTuple):
    """One element kind of the own 16-bit training products: exactly what differs between the kinds."""
    name: str
    autocast: torch.dtype            # the autocast dtype under which the kind is taken
    f32a: str                        # entry points (include/gkg_hip.h): the product on fp32 operands,
    f32a_supported: str              # its envelope,
    planes_bytes: str                # the size of a fragment array
    fragment: torch.dtype            # element type of the fragment arrays
    slots: tuple                     # derived's cache slots of the weight's fragments: (as it is, transposed)
    own_wgrad: bool                  # a weight-gradient kernel of its own (linear_bf16_wgrad): atomics, not under GKG_DETERMINISTIC
    f32a_grouped: str                # the grouped projection (GKG_ENABLE=train_grouped): nb products in one launch,
    f32a_grouped_supported: str      # its envelope
    gslots: tuple                    # derived's cache slots of the grouped weight's stacked fragments: (as it is, transposed)


BF16 = Kind16("bf16", torch.bfloat16, "gkg_linear_bf16_f32a", "gkg_linear_bf16_f32a_supported", "gkg_linear_bf16_planes_bytes",
              torch.bfloat16, ("lin_planes", "lin_planes_t"), True,
              "gkg_linear_bf16_f32a_grouped", "gkg_linear_bf16_f32a_grouped_supported", ("glin_planes", "glin_planes_t"))
F16 = Kind16("f16", torch.float16, "gkg_linear_f16_f32a", "gkg_linear_f16_f32a_supported", "gkg_linear_f16_planes_bytes",
             torch.float16, ("lin_planes_f16", "lin_planes_t_f16"), False,
             "gkg_linear_f16_f32a_grouped", "gkg_linear_f16_f32a_grouped_supported", ("glin_planes_f16", "glin_planes_t_f16"))
KINDS = {k.name: k for k in (BF16, F16)}


def train16_ok(kind, on, x, conv, bn, supported=None) -> bool:
    """Whether ``fused._LinearBNAct.forward`` takes its product from train16_fwd (and the backward its input gradient from
    train16_dgrad and, for a kind with ``own_wgrad``, its weight gradient from linear_bf16_wgrad): the switch, gradients on, not
    GKG_DETERMINISTIC where the kind's own weight gradient adds with atomics, the kind's autocast dtype, an fp32 CUDA matrix with
    unit column stride and a pitch that is a multiple of 4, a dense 1x1 weight over exactly its columns, and the library's answers
    for every product of the kind (``supported(R, cin, cout)`` stands in for them in tests).  ``bn`` takes no part: the BN passes
    behind the product are the caller's, unchanged."""
    if not on:
        return False
    from . import fused
    if not torch.is_grad_enabled() or (kind.own_wgrad and fused.DETERMINISTIC):
        return False
    if not torch.is_autocast_enabled() or torch.get_autocast_dtype("cuda") != kind.autocast:
        return False
    if x.dtype != _F32 or not x.is_cuda or len(x.shape) != 2 or x.stride(1) != 1 or x.stride(0) % 4:
        return False
    wshape = tuple(conv.weight.shape)
    if conv.groups != 1 or len(wshape) != 4 or wshape[2:] != (1, 1) or wshape[1] != x.shape[1]:
        return False
    R, cin, cout = x.shape[0], wshape[1], wshape[0]
    if supported is not None:
        return bool(supported(R, cin, cout))
    lib = _lib.load()
    f32a_supported = getattr(lib, kind.f32a_supported)
    return bool(f32a_supported(R, cin, cout, 0, 1, 0, 0) and f32a_supported(R, cout, cin, 1, 1, 0, 0)
                and (not kind.own_wgrad or lib.gkg_linear_wgrad_bf16_supported(R, cin, cout)))


def _f32a(kind, x, planes, res, R, cin, cout, what):
    """out (R, cout) fp32 = kind(x) (R, cin) . planes (+ res) on the kind's ``*_f32a`` entry point."""
    x = _rows(x, 4)
    if res is not None:
        res = _rows(res, 4)
    out = torch.empty((R, cout), dtype=_F32, device=x.device)
    _lib.check(getattr(_lib.load(), kind.f32a)(_ptr(x), x.stride(0), _ptr(planes), None, None, _ptr(res),
                                               0 if res is None else res.stride(0), _ptr(out), cout, None, 0, R, cin, cout, 0,
                                               _stream()), "%s (%s)" % (kind.f32a, what))
    return out


@torch.no_grad()
def train16_fwd(kind, x, conv):
    """x (R, cin) fp32 -> Y = kind(x) kind(W)^T (R, cout) fp32: the pre-BN matrix (the conv bias stays in the BN passes)."""
    assert x.dtype == _F32 and x.dim() == 2
    cout = conv.weight.shape[0]
    return _f32a(kind, x, derived.lin_planes(conv, kind), None, x.shape[0], x.shape[1], cout, "forward")


@torch.no_grad()
def train16_dgrad(kind, dY, conv, residual=None):
    """dY (R, cout) fp32 -> dx = kind(dY) kind(W) (+ residual (R, cin) fp32: the skip gradient, added in the epilogue) (R, cin)."""
    assert dY.dtype == _F32 and dY.dim() == 2
    w = conv.weight
    cout, cin = w.shape[0], w.numel() // w.shape[0]
    assert dY.shape[1] == cout
    if residual is not None:
        assert residual.dtype == _F32 and tuple(residual.shape) == (dY.shape[0], cin)
    return _f32a(kind, dY, derived.lin_planes(conv, kind, transposed=True), residual, dY.shape[0], cout, cin, "input gradient")


# ---- the GROUPED projection of a Grapher under the same switches plus GKG_ENABLE=train_grouped (``fused.TRAIN_GROUPED``) --------------
# BasicConv's Conv2d(2C -> 2C, 1x1, groups = 4) behind the max-relative aggregation (reference torch_nn.py:57-69 behind
# torch_vertex.py:57-61), reading the XM operand buffer (R, 4 ci): forward and input gradient are ONE launch each of the kind's
# ``*_f32a_grouped`` entry point — no strided gather into a 16-bit copy, no vendor GEMM, no widening pass, no re-layout of dXM.  The
# column permutation (XM's [x chunk | m chunk] order) lives in the cached fragment arrays (derived.glin_planes).  Neither product adds
# atomically, so neither ``own_wgrad`` nor GKG_DETERMINISTIC is asked; the grouped weight gradient stays where _wgrad_grouped puts it.
GROUPS = 4


def train16_grouped_ok(kind, on, XM, conv, bn, supported=None) -> bool:
    """Whether ``fused._GroupedLinearBNAct`` takes its product from train16_grouped_fwd and its input gradient from
    train16_grouped_dgrad: ``on`` (the kind's own switch AND ``fused.TRAIN_GROUPED``: the caller's conjunction), gradients on, the
    kind's autocast dtype, an fp32 CUDA operand buffer XM (R, 4 ci) with unit column stride, a groups = 4 1x1 weight (4 co, ci, 1, 1)
    over exactly those columns, and the library's answers for both products (``supported(R, cin, cout, nb)`` stands in for them in
    tests).  ``bn`` takes no part: the BN passes behind the product are the caller's, unchanged."""
    if not on or not torch.is_grad_enabled():
        return False
    if not torch.is_autocast_enabled() or torch.get_autocast_dtype("cuda") != kind.autocast:
        return False
    if XM.dtype != _F32 or not XM.is_cuda or len(XM.shape) != 2 or XM.stride(1) != 1:
        return False
    wshape = tuple(conv.weight.shape)
    if conv.groups != GROUPS or len(wshape) != 4 or wshape[2:] != (1, 1) or wshape[0] % GROUPS or wshape[1] * GROUPS != XM.shape[1]:
        return False
    R, ci, co = XM.shape[0], wshape[1], wshape[0] // GROUPS
    if supported is None:
        supported = getattr(_lib.load(), kind.f32a_grouped_supported)
    return bool(supported(R, ci, co, GROUPS) and supported(R, co, ci, GROUPS))


def _f32a_grouped(kind, x, ldx, x_gs, planes, out, ldo, out_gs, R, cin, cout, what):
    _lib.check(getattr(_lib.load(), kind.f32a_grouped)(_ptr(x), ldx, x_gs, _ptr(planes), _ptr(out), ldo, out_gs, R, cin, cout, GROUPS,
                                                       _stream()), "%s (%s)" % (kind.f32a_grouped, what))
    return out


@torch.no_grad()
def train16_grouped_fwd(kind, XM, conv):
    """XM (R, 4 ci) fp32, group q's operand its columns [q ci, (q + 1) ci) = [x chunk | m chunk] -> Y (4, R, co) fp32 stacked,
    Y_q = kind(XM_q) kind(Wp_q)^T with Wp = fused._kperm_weight(Wg): the pre-BN matrices (the conv bias stays in the BN passes)."""
    assert XM.dtype == _F32 and XM.dim() == 2
    XM = _rows(XM, 4)
    R, ci, co = XM.shape[0], XM.shape[1] // GROUPS, conv.weight.shape[0] // GROUPS
    Y = torch.empty((GROUPS, R, co), dtype=_F32, device=XM.device)
    return _f32a_grouped(kind, XM, XM.stride(0), ci, derived.glin_planes(conv, kind), Y, co, R * co, R, ci, co, "forward")


@torch.no_grad()
def train16_grouped_dgrad(kind, dY, conv):
    """dY (4, R, co) fp32 stacked -> dXM (R, 4 ci) fp32 written in place, dXM_q = kind(dY_q) kind(Wp_q): columns in XM order."""
    assert dY.dtype == _F32 and dY.dim() == 3 and dY.shape[0] == GROUPS
    dY = dY.contiguous()
    R, co, ci = dY.shape[1], dY.shape[2], conv.weight.shape[1]
    assert co * GROUPS == conv.weight.shape[0]
    dXM = torch.empty((R, GROUPS * ci), dtype=_F32, device=dY.device)
    return _f32a_grouped(kind, dY, co, R * co, derived.glin_planes(conv, kind, transposed=True), dXM, GROUPS * ci, ci, R, co, ci,
                         "input gradient")


@torch.no_grad()
def linear_bf16_wgrad(dY, x, out=None):
    """dW (cout, cin) = bf16(dY)^T bf16(x) over the rows, fp32 accumulation, atomically added slabs (run-dependent order).  ``out``
    as in ``fused._wgrad``'s x6 branch: a gradient-bucket slot is zeroed unless it carries ``_gkg_zero``; without one a fresh
    zeroed tensor."""
    assert dY.dtype == _F32 and x.dtype == _F32 and dY.shape[0] == x.shape[0]
    R, cin, cout = x.shape[0], x.shape[1], dY.shape[1]
    dY, x = _rows(dY, 4), _rows(x, 4)
    if out is not None and (out.dtype != _F32 or not out.is_contiguous() or out.data_ptr() % 16):
        out = None
    if out is None:
        out = torch.zeros((cout, cin), dtype=_F32, device=x.device)
    elif not getattr(out, "_gkg_zero", False):          # a bucket slot cleared by GradBucket.release(prezero=True) is clean
        out.zero_()
    _lib.check(_lib.load().gkg_linear_wgrad_bf16(_ptr(dY), dY.stride(0), _ptr(x), x.stride(0), _ptr(out), R, cin, cout, _stream()),
               "gkg_linear_wgrad_bf16")
    return out
