"""The prepared-token handshake of the k-NN (round 6), host side.

The BN-apply pass that produces a block's tokens also leaves their normalised copies and norms in the workspace of the k-NN call
that reads them next (gkg_bn_apply_knn_prep[_sync], gkg_affine_knn_prep; csrc/gkg_block.hip:proj_apply_prep): a block's fc1
prepares its own QUERIES, a Grapher's fc2 the KEYS of the label graph behind it.  The consumer may set GKG_KNN_X_PREPARED /
GKG_KNN_Y_PREPARED only if the producer ran into the SAME workspace for bit-for-bit the SAME problem — a disagreement does not
crash, it returns a wrong graph.  This module owns that agreement and nothing else: no kernel call (only the size query
gkg_knn_workspace_bytes) and no policy switch — whether tokens are prepared at all (``fused.KNN_PREP``, a patched
``fused.knn_graph_tm``, the bf16 contraction) the callers decide before they come here.

One problem is a ``KnnProblem``.  Three marks carry it from producer to consumer, set and read only here:
  ``_gkg_knn``        on fc1's output (the x half of the XM buffer): the problem whose queries the pass prepared
                      (mark -> consumer_ws_flags);
  ``_gkg_knn_keys``   on a Grapher's token-major companion output: the label graph's problem whose keys fc2's pass prepared
                      (mark -> prepared_keys -> adopt_keys);
  ``_gkg_label_knn``  on the Grapher MODULE in front of a label block: (groups, L, k, dilation, fused_mr) of the label graph, told
                      by the label block on its first step (announce), read by the Grapher from its next call on (announced ->
                      keys_for_label).
"""
from __future__ import annotations

import torch

from . import _lib
from .ops import _ptr


def problem_flags(relative_pos, bf16_contract=False, f16_contract=False) -> int:
    """The flag word of a block's k-NN problem: what producer and consumer compare, and the k-NN call's flags before the _PREPARED bits.
    At most one 16-bit contraction: the library rejects both bits together, and bf16 wins here (fused.knn_contract)."""
    return (_lib.KNN_NORMALIZE | _lib.knn_select_flags() | _lib.relpos_flags(relative_pos)
            | (_lib.KNN_BF16_CONTRACT if bf16_contract else (_lib.KNN_F16_CONTRACT if f16_contract else 0)))


def _workspace(lib, device, B, G, c, N, M, k, d) -> torch.Tensor:
    """A workspace for one fp32 k-NN problem: the one spelling of the size query, for producers and consumers alike."""
    nbytes = lib.gkg_knn_workspace_bytes(B * G, c, N, M, k, d, _lib.F32, _lib.KNN_NORMALIZE)
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


class KnnProblem:
    """One k-NN problem as the C entry points see it: what the producer of the prepared tokens and the k-NN call must agree on for
    the copies in ``ws`` to be THAT call's (same workspace plan, same kernel choice) — the eleven fields of ``tuple()``."""
    __slots__ = ("B", "G", "c", "N", "M", "k", "d", "has_y", "has_rp", "flags", "fused_mr", "ws", "as_keys", "y_ready")

    def __init__(self, B, G, c, N, M, k, d, has_y, relative_pos, fused_mr, flags=None):
        self.B, self.G, self.c, self.N, self.M, self.k, self.d = B, G, c, N, M, k, d
        self.has_y, self.has_rp, self.fused_mr = int(bool(has_y)), int(relative_pos is not None), int(bool(fused_mr))
        self.flags = problem_flags(relative_pos) if flags is None else flags
        self.ws = None           # allocated on first use (workspace), or taken over from the keys' producer (adopt_keys)
        self.as_keys = 0         # 1: this producer call prepares the problem's KEYS (a Grapher's fc2 in front of a GrapherLabel)
        self.y_ready = False     # the keys' copies are already in ``ws`` (the k-NN call then sets GKG_KNN_Y_PREPARED)

    def tuple(self):
        return (self.B, self.G, self.c, self.N, self.M, self.k, self.d, self.has_y, self.has_rp, self.flags, self.fused_mr)

    def workspace(self, lib, device) -> torch.Tensor:
        if self.ws is None:
            self.ws = _workspace(lib, device, self.B, self.G, self.c, self.N, self.M, self.k, self.d)
        return self.ws

    def producer_args(self, lib, out, out_tm, res, ldo, ochunk):
        """The argument run the three producer entry points share, `out` .. `knn_workspace_bytes` (include/gkg_hip.h).  Queries go
        into ``out`` (row pitch ``ldo``, XM chunking ``ochunk``); keys go token-major into ``out_tm``, the same pass adding the
        residual ``res`` and storing the NCHW result in ``out``.  The workspace is allocated here: only by a call that IS a producer."""
        ws, keys = self.workspace(lib, out.device), self.as_keys
        return (_ptr(out_tm if keys else out), 0 if keys else ldo, 0 if keys else ochunk, self.B, self.G, self.c, self.N, self.M,
                self.k, self.d, self.has_y, self.has_rp, self.flags, self.fused_mr, keys, _ptr(res) if keys else None,
                _ptr(out) if keys else None, _ptr(ws), ws.numel())

    def mark(self, out):
        """Producer side, after the pass ran: ``out`` (fc1's output / a Grapher's token-major companion) carries the prepared problem."""
        setattr(out, "_gkg_knn_keys" if self.as_keys else "_gkg_knn", self)

    @classmethod
    def keys_for_label(cls, B, C, N, label_knn):
        """The keys problem a Grapher (B images, N tokens, C channels) prepares for the label graph ``announced`` to it, or None: no
        announcement, or the label graph's groups do not divide C into widths the preparation kernel takes (multiples of 4)."""
        if label_knn is None:
            return None
        G, L, k, d, fused_mr = label_knn
        if C % G or (C // G) % 4:
            return None
        keys = cls(B, G, C // G, L, N, k, d, True, None, fused_mr)
        keys.as_keys = 1
        return keys

    def adopt_keys(self, keys) -> bool:
        """Consumer side of the keys handshake: when the Grapher in front prepared the keys of exactly this problem (``keys``: what
        prepared_keys found), its workspace becomes this problem's — fc1 adds the queries to it."""
        if keys is None or keys.ws is None or keys.tuple() != self.tuple():
            return False
        self.ws, self.y_ready = keys.ws, True
        return True

    def announce(self, producer, groups, L):
        """A label block tells the Grapher module that produced its feature map (None: unknown) which graph it builds over it; the
        Grapher prepares the keys from its next call on.  Stored only when it changed."""
        lk = (groups, L, self.k, self.d, self.fused_mr)
        if producer is not None and producer.__dict__.get("_gkg_label_knn") != lk:
            producer._gkg_label_knn = lk


def announced(module):
    """What a label block announced to this Grapher module (KnnProblem.announce), or None."""
    return module.__dict__.get("_gkg_label_knn")


def prepared_keys(out_tm):
    """The keys problem a Grapher's fc2 left on its token-major output (KnnProblem.mark), or None."""
    return getattr(out_tm, "_gkg_knn_keys", None)


def consumer_ws_flags(lib, x, B, G, c, N, M, k, d, has_y, has_rp, flags, fused_mr):
    """(workspace, flags) for a k-NN call on queries ``x``: the producer's workspace + GKG_KNN_X_PREPARED (+ _Y_PREPARED) when x carries
    prepared copies for exactly this problem (KnnProblem.mark), else a fresh workspace and the flags as given.  The bf16 and fp16
    contractions read no prepared copies."""
    p = getattr(x, "_gkg_knn", None)
    if (p is not None and p.ws is not None and not (flags & (_lib.KNN_BF16_CONTRACT | _lib.KNN_F16_CONTRACT))
            and p.tuple() == (B, G, c, N, M, k, d, int(bool(has_y)), int(bool(has_rp)), flags, int(bool(fused_mr)))):
        return p.ws, flags | _lib.KNN_X_PREPARED | (_lib.KNN_Y_PREPARED if p.y_ready else 0)
    return _workspace(lib, x.device, B, G, c, N, M, k, d), flags
