"""Tensors derived from a layer's parameters and kept between calls — the bf16 weight copy, the BN-folded weight and shifts, the
fragment arrays of the own 16-bit kernels (one builder, ``_fragments``; a projection's four slots behind one ``lin_planes(conv, kind,
transposed)``, the kind a row of linear_bf16.KINDS; a grouped projection's four behind ``glin_planes``), an eval-mode BN's (a, c) — under ONE staleness protocol (``get``), and the
builders of those values.  Mechanism only: which layer takes which of them is decided in ``fused.py``.  The store lives here,
keyed weakly on the owning module: nothing is attached to the module, so deepcopy and pickling do not carry it.  (The x6 weight
planes are not here: planes._WeightPlanes is per device, refreshes in batches and has its own capture rules.)"""
from __future__ import annotations

import weakref

import torch

from . import _lib
from .planes import param_version

_BF16 = torch.bfloat16
_F16 = torch.float16
_STORE = weakref.WeakKeyDictionary()            # owner module -> {slot: ([(weak reference, address, token) per source], (extra, epoch), value)}


def get(owner, slot, sources, build, *, extra=(), stats_of=None, cacheable=True):
    """``build()``'s value for ``owner``'s ``slot``, built again unless every source tensor is the SAME OBJECT at the same address
    with the same planes.param_version token and ``extra`` (plain values: eps, a length) is what it was.  ``stats_of``: a BN whose
    running statistics the value reads — they change behind the version counters, so its ``_gkg_epoch`` (layers._StatsEpoch) joins
    the key, and a norm layer without that counter is never stored.  ``cacheable=False``: build and return, store nothing."""
    epoch = None
    if stats_of is not None:
        epoch = getattr(stats_of, "_gkg_epoch", None)
        cacheable = cacheable and epoch is not None
    if not cacheable:
        return build()
    slots = _STORE.get(owner)
    ent = None if slots is None else slots.get(slot)
    if ent is not None and ent[1] == (extra, epoch) and len(ent[0]) == len(sources):
        for (ref, ptr, version), t in zip(ent[0], sources):           # identity first: it is the cheapest of the three
            if ref() is not t or ptr != t.data_ptr() or version != param_version(t):
                break
        else:
            return ent[2]
    value = build()
    _STORE.setdefault(owner, {})[slot] = ([(weakref.ref(t), t.data_ptr(), param_version(t)) for t in sources], (extra, epoch), value)
    return value


def peek(owner, slot):
    """The stored value, not validated (None: nothing stored)."""
    ent = _STORE.get(owner, {}).get(slot)
    return None if ent is None else ent[2]


def clear(owner=None):
    """Forget what is stored for ``owner`` (None: for every module)."""
    if owner is None:
        _STORE.clear()
    else:
        _STORE.pop(owner, None)


# ---- the fragment arrays of the own 16-bit kernels (include/gkg_hip.h): contraction padded to K_ALIGN, columns to N_ALIGN
K_ALIGN, N_ALIGN = 16, 32


def _up(v, m):
    return (v + m - 1) // m * m


def _fragments(w, k_pad, n_pad, dtype) -> torch.Tensor:
    """w (n, k), or a stack (g, n, k), rounded by ``.to(dtype)`` (autocast's own cast) as [k_pad/8][n_pad][8] (a leading g for a
    stack): fragment (f, n) = w[n][8f .. 8f+7], zero outside the matrix."""
    n, k = w.shape[-2:]
    W = torch.zeros(w.shape[:-2] + (n_pad, k_pad), dtype=dtype, device=w.device)
    W[..., :n, :k] = w.detach().to(dtype)
    return W.view(w.shape[:-2] + (n_pad, k_pad // 8, 8)).transpose(-3, -2).contiguous()


def bf16_fragments(w, k_pad, n_pad) -> torch.Tensor:
    """_fragments in bf16."""
    return _fragments(w, k_pad, n_pad, _BF16)


def f16_fragments(w, k_pad, n_pad) -> torch.Tensor:
    """_fragments in IEEE fp16."""
    return _fragments(w, k_pad, n_pad, _F16)


def _fragments_slot(conv, slot, mat, nbytes, dtype=_BF16):
    """``mat(w)`` -> the matrix (or stack) to lay out, ``nbytes(lib, n, k)`` -> the library's size of that array."""
    def build():
        m = mat(conv.weight.detach())
        n, k = m.shape[-2:]
        planes = _fragments(m, _up(k, K_ALIGN), _up(n, N_ALIGN), dtype)
        assert planes.numel() * 2 == int(nbytes(_lib.load(), n, k)), (slot, tuple(m.shape))      # the library owns the paddings
        return planes
    return get(conv, slot, (conv.weight,), build)


def lin_planes(conv, kind="bf16", transposed=False) -> torch.Tensor:
    """The projection's UNFOLDED weight (cout, cin) as the fragment array the own projection kernels stream, [ci_pad/8][co_pad][8]:
    gkg_linear_bf16 and its kin, and a training layer's forward.  ``kind``: a row of linear_bf16.KINDS or its name — the element
    type, the library's size question and the two slots are the row's.  ``transposed``: the array of W^T instead, what the input
    gradient dx = dY W streams (the ``*_f32a`` entry point with contraction cout and output columns cin): [co_pad'/8][ci_pad'][8],
    fragment (f, n) = w[8f .. 8f+7][n]."""
    if isinstance(kind, str):
        kind = linear_bf16.KINDS[kind]
    return _fragments_slot(conv, kind.slots[transposed],
                           lambda w: w.reshape(w.shape[0], -1).t() if transposed else w.reshape(w.shape[0], -1),
                           lambda lib, n, k: getattr(lib, kind.planes_bytes)(k, n), kind.fragment)


def kperm_weight(Wg: torch.Tensor) -> torch.Tensor:
    """(nb, co, ci) grouped weight with its input columns as [even | odd]: the order an XM operand buffer presents them in (the x
    chunk, then the m chunk).  (``fused._kperm_weight`` is this function.)"""
    nb, co, ci = Wg.shape
    return Wg.view(nb, co, ci // 2, 2).permute(0, 1, 3, 2).reshape(nb, co, ci)


def glin_planes(conv, kind="bf16", transposed=False) -> torch.Tensor:
    """The GROUPED projection's weight (nb co, ci, 1, 1), nb = conv.groups, as the stacked fragment array the ``*_f32a_grouped`` entry
    points stream: [nb][..] — nb arrays of lin_planes' layout back to back, of Wp[q] (co, ci) = kperm_weight(Wg)[q] for the forward
    (contraction columns in XM order) or, ``transposed``, of Wp[q]^T (ci, co) for the input gradient (output columns in XM order).
    ``kind`` as in lin_planes; the slots are the row's ``gslots``, the size the library's: nb x planes_bytes (asked for the widths
    rounded up to the kernels' granule of 8, which pads the same: a width the kernels refuse still has its array)."""
    if isinstance(kind, str):
        kind = linear_bf16.KINDS[kind]
    nb = conv.groups

    def mat(w):
        Wp = kperm_weight(w.reshape(nb, w.shape[0] // nb, -1))
        return Wp.transpose(1, 2) if transposed else Wp
    return _fragments_slot(conv, kind.gslots[transposed], mat,
                           lambda lib, n, k: nb * getattr(lib, kind.planes_bytes)(_up(k, 8), _up(n, 8)), kind.fragment)


def mr_planes(conv) -> torch.Tensor:
    """The 4-group projection's weight (4 co, ci) as the fragment array gkg_mr_linear_bf16 streams: [4][ci_pad/8][co_pad][8]."""
    return _fragments_slot(conv, "mr_planes", lambda w: w.reshape(4, w.shape[0] // 4, w.shape[1]),
                           lambda lib, co, ci: lib.gkg_mr_linear_planes_bytes(4 * ci // 2))


# ---- weight copies
def w16(conv) -> torch.Tensor:
    """bf16 copy of a projection's weight (inference: cast once, not per call)."""
    return get(conv, "w16", (conv.weight,), lambda: conv.weight.detach().to(_BF16))


def folded(conv, bn):
    """Inference (eval-mode BN): the BN scale folded into a bf16 copy of the weight and the shift (conv bias and running mean
    included) in both precisions — (W' (cout, cin) bf16, c' (cout) bf16, c' fp32).  With them out = act(x W'^T + c') is ONE
    library GEMM with a bias(+GELU) epilogue."""
    def build():
        with torch.no_grad():
            a = bn.weight.float() * torch.rsqrt(bn.running_var.float() + bn.eps)
            shift = bn.bias.float() - a * bn.running_mean.float()
            if conv.bias is not None:
                shift = shift + a * conv.bias.float()
            wf = (conv.weight.float().view(conv.weight.shape[0], -1) * a.view(-1, 1)).to(_BF16).contiguous()
            return wf, shift.to(_BF16).contiguous(), shift.contiguous()
    srcs = (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var) + (() if conv.bias is None else (conv.bias,))
    return get(conv, "folded", srcs, build, extra=(bn.eps,), stats_of=bn)


from . import linear_bf16      # noqa: E402  (last: linear_bf16 imports this module; only its KINDS is read, when lin_planes is called)
