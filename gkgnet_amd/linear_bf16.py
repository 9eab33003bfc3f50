"""bf16 inference: a dense 1x1 projection with its eval-mode BN (+ GELU) (+ residual) as ONE launch of the library's own kernel
(gkg_linear_bf16, csrc/gkg_linear_bf16.hip) — the weight's fragment array, the call, and the predicate ``fused._lin`` asks before
it dispatches here.  Mechanism only: the switch (``fused.LIN_BF16``) and the mode test (``fused.lowp_inference``) stay in
``fused.py`` and arrive as arguments."""
from __future__ import annotations

import torch

from . import _lib, bn_passes
from .ops import _ptr, _stream
from .planes import param_version

_F32 = torch.float32


def _lin_planes_of(conv) -> torch.Tensor:
    """The projection's UNFOLDED weight as the bf16 fragment array gkg_linear_bf16 streams: [ci_pad/8][co_pad][8], fragment
    (f, n) = w[n][8f .. 8f+7], zero outside (include/gkg_hip.h) — cached on the module and rebuilt when the parameter changes."""
    w = conv.weight
    ent = getattr(conv, "_gkg_linplanes", None)
    if ent is None or ent[0] != param_version(w) or ent[1] != w.data_ptr():
        co, ci = w.shape[0], w.numel() // w.shape[0]
        nbytes = int(_lib.load().gkg_linear_bf16_planes_bytes(ci, co))       # the library owns the paddings
        ci_pad = (ci + 15) // 16 * 16
        co_pad = nbytes // (2 * ci_pad) if nbytes else 0
        assert nbytes and co_pad >= co and co_pad * ci_pad * 2 == nbytes, (ci, co, nbytes)
        W = torch.zeros((co_pad, ci_pad), dtype=torch.bfloat16, device=w.device)
        W[:co, :ci] = w.detach().reshape(co, ci).to(torch.bfloat16)
        planes = W.view(co_pad, ci_pad // 8, 8).permute(1, 0, 2).contiguous()
        assert planes.numel() * 2 == nbytes
        ent = (param_version(w), w.data_ptr(), planes)
        conv._gkg_linplanes = ent
    return ent[2]


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
    _lib.check(lib.gkg_linear_bf16(_ptr(x16), x16.stride(0), _ptr(_lin_planes_of(conv)), _ptr(a), _ptr(c), _ptr(residual),
                                   0 if residual is None else residual.stride(0), _ptr(o32), cout, _ptr(o16), cout, R, cin, cout,
                                   act, _stream()), "gkg_linear_bf16")
    return o32, o16
