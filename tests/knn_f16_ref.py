"""Plain restatement of the k-NN whose distance product runs on the fp16 matrix cores (include/gkg_hip.h: GKG_KNN_F16_CONTRACT), and the
bound the kernels are held to.  The sibling of tests/knn_bf16_ref.py (``R``): inputs (``R.FORMS``, ``R.make_case``), judge and near-tie
share are that module's; only the element format of the planes differs.

DEFINITION (csrc/gkg_knn_prep.h, the ``S.tb`` branch of token_prep_body with HF; csrc/gkg_knn_tile.h, the ``BF`` branches with
KNN_EL_F16).  Token preparation is the contract's, normalised (the flag is rejected without GKG_KNN_NORMALIZE):
    s = fmaf-chain t^2,  den = max(sqrtf(s), 1e-12),  th = t / den,  sq = fmaf-chain th^2
(``O.token_prep``); the planes hold h(th) = fp16 round-to-nearest-even of the fp32 th with a result of magnitude below 2^-14 (an fp16
subnormal) replaced by +0; sq is taken from the unrounded th.
    dist(n, m) = ( relpos[n][m] + sum_ch (-2 h(xh[n][ch])) h(yh[m][ch]) ) + sqy[m]              (the query's |x|^2 is left out)
Neighbours: the k d smallest (dist, m) pairs, smaller index first on equal distance; ranks 0, d, 2d, ... are emitted.  ``reference``
evaluates dist in fp64 as R.reference does; a NaN distance is ranked as +inf.

BOUND.  R's derivation carries over.  The products are exact in fp32: two 11-bit significands give at most 22 bits, and with every
nonzero |h| >= 2^-14 a product is at least 2^-27 in magnitude with its last bit at 2^-48 or above — far inside fp32's range.  What the
hardware is free in is the order of the c + 1 fp32 additions; every partial sum is at most max|rp| + 2 |h xh| |h yh| + sqy
<= max|rp| + 3.1 (|th| <= 1 + c 2^-24, h adds 2^-12 relative, sq <= 1 + 2 c 2^-24).  So |kernel dist - dist| <= E = (c + 2) 2^-24
(max|rp| + 3.1), and two implementations within E differ at a rank only by keys whose definition distances are within 2 E.

``h`` is written out on the bits of the fp32 value (no library conversion), so that tests/test_knn_f16_reference_host.py can hold it
against torch's.  A helper module, not a test module and not a conftest; it imports nothing of the package."""
import numpy as np
import torch

import knn_bf16_ref as R

FORMS, NEAR_TIE_CAP = R.FORMS, R.NEAR_TIE_CAP
shape_id, make_case, to_tm, bound, judge, near_tie_share = R.shape_id, R.make_case, R.to_tm, R.bound, R.judge, R.near_tie_share

F16_MIN_NORMAL = 2.0 ** -14


def h(a):
    """fp32 array -> the fp64 value of its fp16 round-to-nearest-even with subnormal results flushed to +0 (NaN stays NaN, +-inf stay).
    A magnitude in [2^-14 - 2^-25, 2^-14) rounds UP to the normal 2^-14 (the tie goes to the even neighbour, which is 2^-14) and is
    kept; anything smaller would be a subnormal or zero and becomes +0."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    bits = a.view(np.uint32)
    mag = bits & np.uint32(0x7FFFFFFF)
    r = mag + np.uint32(0xFFF) + ((mag >> np.uint32(13)) & np.uint32(1))          # nearest-even on the 13 dropped significand bits
    r = r & np.uint32(0xFFFFE000)
    val = r.view(np.float32).astype(np.float64)
    val = np.where(val >= 65520.0, np.inf, val)                                   # past the largest fp16 (65504): overflow
    absa = np.abs(a.astype(np.float64))
    small = absa < F16_MIN_NORMAL
    val = np.where(small, np.where(absa >= F16_MIN_NORMAL - 2.0 ** -25, F16_MIN_NORMAL, 0.0), val)
    val = np.where(val == 0.0, 0.0, np.copysign(val, a.astype(np.float64)))       # the flush gives +0
    val = np.where(np.isfinite(a), val, a.astype(np.float64))
    return torch.from_numpy(val)


def flushed_share(a):
    """Share of the NONZERO values of the fp32 array that the definition's flush sends to +0."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    nz = a != 0
    return float(((h(a).numpy() == 0) & nz).sum()) / max(int(nz.sum()), 1)


def prepared(x, y):
    """-> h(xh) (BG, c, N), h(yh) (BG, c, M), sqy (BG, M), all fp64 tensors, from the C oracle's token preparation (normalised)."""
    from oracle import c_oracle as O
    xh, sqx = O.token_prep(x, True)
    if y is None:
        yh, sqy = xh, sqx
    else:
        yh, sqy = O.token_prep(y, True)
    return h(xh), h(yh), torch.from_numpy(sqy).double()


def reference(x, y, rp, k, d, device="cpu", keep_D=True, values_only=False):
    """R.reference with h() in place of bf(): x (BG, c, N), y (BG, c, M) or None, rp (N, M) or None (numpy fp32) -> (D, topd, topi) on
    ``device``; D (BG, N, M) fp64 with NaN replaced by +inf (None unless keep_D), topd / topi (BG, N, min(k d + 1, M)) ascending, ties
    by index (``values_only``: torch.topk, for callers that read topd alone)."""
    xb, yb, sqy = prepared(x, y)
    BG, M = sqy.shape
    take = min(k * d + 1, M)
    rp64 = None if rp is None else torch.from_numpy(np.ascontiguousarray(rp)).double().to(device)
    Ds, tds, tis = [], [], []
    for bg in range(BG):
        D = -2.0 * (xb[bg].to(device).t() @ yb[bg].to(device))
        if rp64 is not None:
            D = D + rp64
        D = D + sqy[bg].to(device)[None, :]
        D = torch.where(torch.isnan(D), torch.full_like(D, float("inf")), D)
        if values_only:
            td, ti = torch.topk(D, take, dim=-1, largest=False, sorted=True)
        else:
            sd, si = torch.sort(D, dim=-1, stable=True)
            td, ti = sd[:, :take].contiguous(), si[:, :take].contiguous()
        tds.append(td)
        tis.append(ti)
        if keep_D:
            Ds.append(D)
    return (torch.stack(Ds) if keep_D else None), torch.stack(tds), torch.stack(tis)
