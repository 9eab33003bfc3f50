"""Plain restatement of the k-NN whose distance product runs on the bf16 matrix cores (include/gkg_hip.h: GKG_KNN_BF16_CONTRACT), the
bound the kernels are held to, and the inputs the tests share.

DEFINITION (csrc/gkg_knn_prep.h, the ``S.tb`` branch of token_prep_body; csrc/gkg_knn_tile.h, the ``BF`` branches).  Per token
    s = fmaf-chain t^2,  den = max(sqrtf(s), 1e-12),  th = t / den,  sq = fmaf-chain th^2          (GKG_KNN_NORMALIZE; else th = t)
which is oracle/gkg_oracle.c's token_prep bit for bit (``O.token_prep``); the planes hold bf(th) = bf16 round-to-nearest-even of the
fp32 th, sq is taken from the unrounded th.  The tile kernel's accumulator starts at relative_pos[n][m] (0 without a bias), takes the
exact products (-2 bf(xh[n][ch])) bf(yh[m][ch]) in fp32 and the key's squared norm is added last:
    dist(n, m) = ( relpos[n][m] + sum_ch (-2 bf(xh[n][ch])) bf(yh[m][ch]) ) + sqy[m]            (the query's |x|^2 is left out)
Neighbours: the k d smallest (dist, m) pairs, smaller index first on equal distance; ranks 0, d, 2d, ... are emitted.
``reference`` evaluates dist in fp64 (every product and the sum of a row are exact to 2^-53 relative: the fp64 value IS the
definition's real-number value for the purposes of a 2^-24 bound).  A NaN distance (non-finite inputs) never enters a list — the
kernel's insert compares with '<' — and is ranked as +inf here.

BOUND.  The only freedom the hardware has is the order of the c + 1 fp32 additions of a distance (c products onto the accumulator, in
16-deep steps whose inner order is the matrix core's, then sqy).  Each addition rounds a partial sum to fp32: relative error 2^-24,
and every partial sum is at most max|rp| + 2 |bf xh| |bf yh| + sqy <= max|rp| + 3.1 in magnitude (normalised tokens: |th| <= 1 + c 2^-24,
bf rounding adds 2^-9 relative, sq <= 1 + 2 c 2^-24).  So |kernel dist - dist| <= E = (c + 2) 2^-24 (max|rp| + 3.1): one unit of
slack over the c + 1 additions.  Without GKG_KNN_NORMALIZE the same with 2 max|bf x| max|bf y| + max sqy in place of 3.1 (``scale``).
Two implementations that each compute dist within E can differ at a rank only by keys whose definition distances are within 2 E.

A helper module, not a test module and not a conftest; it imports nothing of the package."""
import numpy as np
import torch

# (B, G, c, N, M (None = self graph), k, d, bias): the forms of knn_plan's 16-bit branch (csrc/gkg_knn_plan.h); see tests/test_hip_knn_bf16_abi.py
FORMS = [(2, 1, 12, 77, None, 3, 2, True), (2, 4, 80, 324, None, 9, 1, True), (2, 2, 40, 80, 1000, 9, 1, False),
         (8, 1, 40, 4100, 300, 9, 2, True), (32, 1, 12, 4100, 520, 9, 1, True), (32, 1, 12, 4100, 520, 18, 1, False),
         (1, 2, 200, 300, None, 9, 2, True), (1, 1, 320, 200, None, 9, 3, True), (1, 1, 320, 200, None, 9, 2, True),
         (2, 1, 48, 300, None, 18, 2, True), (1, 1, 16, 100, 333, 32, 2, False), (1, 1, 33, 65, 130, 5, 1, True)]
NEAR_TIE_CAP = 0.05          # condition on the inputs of every FORMS case (tests/test_knn_bf16_reference_host.py)


def shape_id(s):
    return "x".join("self" if v is None else ("bias" if v is True else ("nobias" if v is False else str(v))) for v in s)


def make_case(shape, seed=0):
    """-> dict: shape, x (BG, c, N) fp32, y (BG, c, M) fp32 or None (self graph), rp (N, M) fp32 in [-1, 0] or None, M."""
    B, G, c, N, M_, k, d, bias = shape
    M = N if M_ is None else M_
    rng = np.random.default_rng([seed, B, G, c, N, M, k, d, int(bias)])
    x = rng.standard_normal((B * G, c, N)).astype(np.float32)
    y = None if M_ is None else rng.standard_normal((B * G, c, M)).astype(np.float32)
    rp = -rng.random((N, M)).astype(np.float32) if bias else None
    return dict(shape=shape, x=x, y=y, rp=rp, M=M)


def to_tm(a, B):
    """(B G, c, T) -> (B, T, C = G c): channel g c + ch of token t is group g's channel ch."""
    BG, c, T = a.shape
    return np.ascontiguousarray(a.reshape(B, (BG // B) * c, T).transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------------------------------ reference
def bf(a):
    """fp32 array -> the fp64 value of its bf16 round-to-nearest-even (NaN stays NaN)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().double()


def prepared(x, y, normalize=True):
    """-> bf(xh) (BG, c, N), bf(yh) (BG, c, M), sqy (BG, M), all fp64 tensors, from the C oracle's token preparation."""
    from oracle import c_oracle as O
    xh, sqx = O.token_prep(x, normalize)
    if y is None:
        yh, sqy = xh, sqx
    else:
        yh, sqy = O.token_prep(y, normalize)
    return bf(xh), bf(yh), torch.from_numpy(sqy).double()


def reference(x, y, rp, k, d, normalize=True, device="cpu", keep_D=True, values_only=False):
    """x (BG, c, N), y (BG, c, M) or None, rp (N, M) or None (numpy fp32) -> (D, topd, topi) on ``device``:
    D (BG, N, M) fp64 distances of the definition with NaN replaced by +inf (None unless keep_D), topd / topi (BG, N, min(k d + 1, M))
    the smallest distances in ascending order, ties by index (a stable sort of every row; ``values_only``: torch.topk, whose order of
    equal distances is unspecified — for callers that read topd alone).  One problem at a time."""
    xb, yb, sqy = prepared(x, y, normalize)
    BG, M = sqy.shape
    kd = k * d
    take = min(kd + 1, M)
    rp64 = None if rp is None else torch.from_numpy(np.ascontiguousarray(rp)).double().to(device)
    Ds, tds, tis = [], [], []
    for bg in range(BG):
        X, Y = xb[bg].to(device), yb[bg].to(device)
        D = -2.0 * (X.t() @ Y)
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


def scale(x, y, normalize=True):
    """The bound on 2 |bf xh| |bf yh| + sqy of a case: 3.1 for normalised tokens, the case's own maxima otherwise."""
    if normalize:
        return 3.1
    xb, yb, sqy = prepared(x, y, False)
    fin = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)        # noqa: E731
    nx, ny = fin(xb).pow(2).sum(1).sqrt().max(), fin(yb).pow(2).sum(1).sqrt().max()
    return float(2.0 * nx * ny + fin(sqy).max())


def bound(c, rp, scale=3.1):
    """E: how far a kernel distance may lie from the definition's (module docstring)."""
    rmax = 0.0 if rp is None else float(np.abs(rp).max())
    return (c + 2) * 2.0 ** -24 * (rmax + scale)


def judge(got, D, topd, topi, k, d, E, rows=None, what=""):
    """got (BG, N, k) integer tensor (any device) against the reference.  Asserted: every index in [0, M); the k entries of a row
    distinct; at every kept rank j |D[n, got[n, j]] - topd[n, j d]| <= 2 E.  ``rows`` (BG, N) bool: the rows the last two are
    asked of (default all).  -> (share of the judged positions where got != topi, largest tolerated gap / 2 E)."""
    M = D.shape[2]
    got = got.to(D.device).long()
    assert got.shape == (D.shape[0], D.shape[1], k), (got.shape, D.shape, k)
    assert int(got.min()) >= 0 and int(got.max()) < M, f"{what}: index outside [0, {M}): min {int(got.min())}, max {int(got.max())}"
    if rows is None:
        rows = torch.ones(got.shape[:2], dtype=torch.bool, device=D.device)
    rows = rows.to(D.device)
    srt = torch.sort(got, dim=-1).values
    dup = (srt[..., 1:] == srt[..., :-1]).any(-1) & rows
    assert not bool(dup.any()), f"{what}: {int(dup.sum())} rows name a key twice, first {torch.nonzero(dup)[0].tolist()}"
    want_d, want_i = topd[..., 0:k * d:d], topi[..., 0:k * d:d]
    gap = (torch.gather(D, 2, got) - want_d).abs()
    gap = torch.where(rows[..., None], gap, torch.zeros_like(gap))
    bad = ~(gap <= 2 * E)                                                       # a NaN gap is bad
    if bool(bad.any()):
        b, n, j = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} positions beyond 2E = {2 * E:.3e}; first (bg={b}, n={n}, rank={j * d}): key "
                             f"{int(got[b, n, j])} at {float(D[b, n, got[b, n, j]]):.9f}, reference key {int(want_i[b, n, j])} at "
                             f"{float(want_d[b, n, j]):.9f} (gap / 2E = {float(gap[b, n, j]) / (2 * E):.2f}; worst "
                             f"{float(torch.nan_to_num(gap, nan=float('inf')).max()) / (2 * E):.2f})")
    mism = (got != want_i) & rows[..., None]
    total = int(rows.sum()) * k
    worst = float(gap[mism].max()) / (2 * E) if bool(mism.any()) else 0.0
    return int(mism.sum()) / max(total, 1), worst


def near_tie_share(topd, E, k, d):
    """Share of the kept positions (ranks 0, d, 2d, ...) whose reference distance lies within 2 E of the rank before or after it;
    topd (BG, N, min(k d + 1, M)).  A property of the inputs alone; every mismatch ``judge`` tolerates is one of these positions."""
    diff = (topd[..., 1:] - topd[..., :-1]) <= 2 * E                            # diff[r]: ranks r and r + 1 are near
    kd = k * d
    pad = torch.zeros_like(diff[..., :1])
    after = torch.cat([diff, pad], -1)[..., :kd]                                # rank r near rank r + 1 (r + 1 may be rank k d)
    before = torch.cat([pad, diff], -1)[..., :kd]                               # rank r near rank r - 1
    near = (after | before)[..., 0:kd:d]
    return float(near.double().mean())
