"""tests/knn_bf16_ref.py — the reference the GPU test tests/test_hip_knn_bf16_abi.py holds the bf16-contraction k-NN to — pinned
on the CPU, together with the one condition that test puts on its inputs.

TOKEN PREPARATION.  ``O.token_prep`` (oracle/gkg_oracle.c's token_prep, exported) against fp64: th within 2 ulp of x / |x|, sq
within c 2^-23 of sum th^2, a zero token gives zeros, without normalisation th is x bit for bit.
RANKING.  A 1 x 2 x 3 x 4 problem of small integers (every value a bf16 number, no normalisation) whose distances and ranking are
written out below, ties included.
CONDITION.  For every shape of ``R.FORMS``: at most 5 % of the kept positions lie within 2 E of a neighbouring rank.  The GPU test
tolerates a differing neighbour only at such positions, so the cap bounds what its tolerance could hide.  A condition on the
inputs, not a measurement of a kernel: a seed that lands above it is replaced, the cap stays."""
import numpy as np
import pytest
import torch

import knn_bf16_ref as R
from oracle import c_oracle as O


# ------------------------------------------------------------------------------------------------------------------ token_prep
@pytest.mark.parametrize("c", (12, 40, 320))
def test_token_prep_against_fp64(c):
    """th = t / max(sqrtf(s), 1e-12) with s an fmaf chain of c squares: the chain is within c 2^-24 of sum t^2 relative (c roundings),
    the square root halves that and adds 2^-24, the division adds 2^-24: |th - x / |x|| <= (2 + c / 2) 2^-24 |th|, asserted at every
    width.  At the narrowest width of the GPU test's table (c = 12) the chain's own error stays below one rounding and th is
    within 2 ulp; at c = 40 this generator's worst token is 2.9 ulp off — the chain, not a defect — so 2 ulp is asked of c = 12 alone."""
    rng = np.random.default_rng(c)
    x = rng.standard_normal((3, c, 50)).astype(np.float32)
    x[1, :, 7] = 0.0                                                           # an all-zero token
    th, sq = O.token_prep(x, normalize=True)
    x64 = x.astype(np.float64)
    nrm = np.sqrt((x64 ** 2).sum(1, keepdims=True))
    want = np.divide(x64, nrm, out=np.zeros_like(x64), where=nrm > 0)
    err = np.abs(th.astype(np.float64) - want)
    ulps = err / np.spacing(np.abs(th)).astype(np.float64)
    print(f"token_prep c={c}: th worst {ulps.max():.2f} ulp, worst err / bound {(err / ((2 + c / 2) * 2.0 ** -24 * np.abs(want) + 1e-300)).max():.3f}")
    assert (err <= (2 + c / 2) * 2.0 ** -24 * np.abs(want)).all()
    if c == 12:
        assert ulps.max() <= 2.0
    s64 = (th.astype(np.float64) ** 2).sum(1)
    assert np.abs(sq.astype(np.float64) - s64).max() <= c * 2.0 ** -23
    assert not th[1, :, 7].any() and sq[1, 7] == 0.0
    assert np.abs(s64 - 1.0)[(nrm > 0)[:, 0, :]].max() <= 4 * c * 2.0 ** -24                    # the tokens ARE normalised


def test_token_prep_without_normalisation():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 24, 33)).astype(np.float32)
    x[0, :, 3] = 0.0
    th, sq = O.token_prep(x, normalize=False)
    assert np.array_equal(th.view(np.int32), x.view(np.int32))
    s64 = (x.astype(np.float64) ** 2).sum(1)
    assert (np.abs(sq.astype(np.float64) - s64) <= 24 * 2.0 ** -23 * s64).all()
    assert sq[0, 3] == 0.0


# ------------------------------------------------------------------------------------------------------------------ ranking
def test_hand_made_problem():
    """dist(n, m) = rp[n][m] - 2 x_n . y_m + |y_m|^2:
         queries (1,0) (0,1) (1,1);  keys (1,0) (0,2) (1,1) (-1,0), |y|^2 = 1 4 2 1;  rp = 0 except rp[0][3] = -4.5
         n = 0:  -1   4   0  -1.5     ranking 3 0 2 1
         n = 1:   1   0   0   1       ranking 1 2 0 3   (two exact ties: smaller index first)
         n = 2:  -1   0  -2   3       ranking 2 0 1 3"""
    x = np.array([[[1, 0, 1], [0, 1, 1]]], np.float32)                          # (1, 2, 3)
    y = np.array([[[1, 0, 1, -1], [0, 2, 1, 0]]], np.float32)                   # (1, 2, 4)
    rp = np.zeros((3, 4), np.float32)
    rp[0, 3] = -4.5
    D, topd, topi = R.reference(x, y, rp, 2, 2, normalize=False)
    assert D[0].tolist() == [[-1, 4, 0, -1.5], [1, 0, 0, 1], [-1, 0, -2, 3]]
    assert topi[0].tolist() == [[3, 0, 2, 1], [1, 2, 0, 3], [2, 0, 1, 3]]
    assert topd[0].tolist() == [[-1.5, -1, 0, 4], [0, 0, 1, 1], [-2, -1, 0, 3]]
    E = R.bound(2, rp, R.scale(x, y, normalize=False))
    assert E == 4 * 2.0 ** -24 * (4.5 + (2 * np.sqrt(2.0) * 2.0 + 4.0))
    want = torch.tensor([[[3, 2], [1, 0], [2, 1]]])                               # ranks 0 and 2
    assert R.judge(want, D, topd, topi, 2, 2, E) == (0.0, 0.0)
    # the tied pair the other way round is a mismatch judge tolerates (gap 0); a key at another distance is not
    assert R.judge(torch.tensor([[[3, 2], [2, 3], [2, 1]]]), D, topd, topi, 2, 2, E) == (2 / 6, 0.0)
    with pytest.raises(AssertionError, match="beyond 2E"):
        R.judge(torch.tensor([[[3, 1], [1, 0], [2, 1]]]), D, topd, topi, 2, 2, E)
    with pytest.raises(AssertionError, match="twice"):
        R.judge(torch.tensor([[[3, 3], [1, 0], [2, 1]]]), D, topd, topi, 2, 2, E)
    with pytest.raises(AssertionError, match="outside"):
        R.judge(torch.tensor([[[3, 4], [1, 0], [2, 1]]]), D, topd, topi, 2, 2, E)
    # near ties: k = 3, d = 1 keeps ranks 0, 1, 2 and looks at rank 3 — row 1 has all three near a neighbour, the others none
    _, topd3, _ = R.reference(x, y, rp, 3, 1, normalize=False)
    assert R.near_tie_share(topd3, E, 3, 1) == 3 / 9
    assert R.near_tie_share(topd, E, 2, 2) == 2 / 6                              # ranks 0 and 2 of row 1 (k d == M: no rank after)


def test_a_nan_distance_ranks_last():
    x = np.array([[[1, 0], [0, 1]]], np.float32)
    y = np.array([[[np.nan, 0, 1], [0, 1, 1]]], np.float32)
    D, topd, topi = R.reference(x, y, None, 2, 1, normalize=False)
    assert topi[0].tolist() == [[2, 1, 0], [1, 2, 0]] and bool(torch.isinf(D[0, :, 0]).all())


# ------------------------------------------------------------------------------------------------------------------ condition
@pytest.mark.parametrize("shape", R.FORMS, ids=R.shape_id)
def test_inputs_keep_near_ties_rare(shape):
    B, G, c, N, M_, k, d, bias = shape
    case = R.make_case(shape)
    _, topd, _ = R.reference(case["x"], case["y"], case["rp"], k, d, keep_D=False, values_only=True)
    share = R.near_tie_share(topd, R.bound(c, case["rp"]), k, d)
    print(f"near-tie share {R.shape_id(shape)}: {100 * share:.2f} %")
    assert share <= R.NEAR_TIE_CAP
