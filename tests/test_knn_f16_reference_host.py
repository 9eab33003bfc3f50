"""tests/knn_f16_ref.py — the reference the GPU test tests/test_hip_knn_f16_abi.py holds the fp16-contraction k-NN
(GKG_KNN_F16_CONTRACT) to — pinned on the CPU, together with the one condition that test puts on its inputs.

ROUNDING.  ``H.h`` — fp16 round-to-nearest-even written out on the fp32 bits, subnormal results flushed to +0 — against torch's
conversion wherever that gives a normal number, zero or a non-finite value, and at the flush boundary: 2^-15 flushes, 2^-14 does not,
the fp32 values just below 2^-14 that round up to it are kept.
RANKING.  A 1 x 2 x 3 x 4 problem whose normalised values are fp16 numbers; distances and ranking are written out below, with an exact
tie.
CONDITION.  For every shape of ``R.FORMS`` (the existing seeds): at most 5 % of the kept positions lie within 2 E of a neighbouring
rank of the fp16 definition's distances.  The GPU test tolerates a differing neighbour only at such positions."""
import numpy as np
import pytest
import torch

import knn_bf16_ref as R
import knn_f16_ref as H


# ------------------------------------------------------------------------------------------------------------------ rounding
def test_flush_boundary():
    v = np.array([2.0 ** -15, -2.0 ** -15, 2.0 ** -14, -2.0 ** -14, 2.0 ** -24, 3e-5, -3e-5, 0.0, -0.0], np.float32)
    got = H.h(v)
    assert got.tolist() == [0.0, 0.0, 2.0 ** -14, -2.0 ** -14, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert not bool(torch.signbit(got[[0, 1, 4, 5, 6, 7, 8]]).any()), "a flushed value is +0"
    # the largest fp32 below 2^-14 lies within half an fp16 subnormal step (2^-25) of it: the rounded result is the normal 2^-14
    below = np.nextafter(np.float32(2.0 ** -14), np.float32(0))
    assert H.h(np.array([below, -below])).tolist() == [2.0 ** -14, -2.0 ** -14]
    assert torch.tensor([below]).half().double().item() == 2.0 ** -14
    # ... the tie itself too (to the even neighbour), one fp32 step below the tie does not
    tie = np.float32(2.0 ** -14 - 2.0 ** -25)
    assert H.h(np.array([tie])).item() == 2.0 ** -14 and torch.tensor([tie]).half().double().item() == 2.0 ** -14
    assert H.h(np.array([np.nextafter(tie, np.float32(0))])).item() == 0.0
    assert H.flushed_share(np.array([0.0, 3e-5, 0.5, 2.0 ** -14], np.float32)) == 1 / 3


def test_h_agrees_with_torch_half_on_normal_results():
    rng = np.random.default_rng(0)
    mant = rng.random(400000).astype(np.float32) + 1.0
    expo = rng.integers(-20, 17, 400000)
    v = (np.ldexp(mant, expo) * rng.choice([-1.0, 1.0], 400000)).astype(np.float32)
    # ties and their fp32 neighbours at several exponents, the overflow threshold, non-finite values
    ties = np.array([(1 + (2 * j + 1) * 2.0 ** -11) * 2.0 ** e for j in (0, 1, 2, 511) for e in (-14, -3, 0, 15)], np.float32)
    edge = np.concatenate([ties, np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(np.inf)),
                           np.array([65504.0, 65519.99, 65520.0, 1e6, np.inf, -np.inf, np.nan, 0.0, 1.0, -1.0], np.float32)])
    v = np.concatenate([v, edge, -edge])
    want = torch.from_numpy(v).half()
    got = H.h(v)
    normal = (want.abs().double() >= 2.0 ** -14) | (want == 0) | ~torch.isfinite(want)
    assert int(normal.sum()) > 300000 and int((~normal).sum()) > 10000
    same = (got == want.double()) | (torch.isnan(got) & torch.isnan(want))
    assert bool(same[normal & (torch.from_numpy(v) != 0) | ~torch.isfinite(want)].all())
    # where torch gives a subnormal (or rounds a nonzero value to zero) the definition gives +0
    sub = ~normal | ((want == 0) & (torch.from_numpy(v) != 0))
    assert bool((got[sub] == 0).all()) and not bool(torch.signbit(got[sub]).any())


# ------------------------------------------------------------------------------------------------------------------ ranking
def test_hand_made_problem():
    """Unit axis vectors: already normalised, every value an fp16 number, so the planes hold the inputs themselves.
         queries (1,0) (0,1) (0,-1);  keys (1,0) (0,1) (-1,0) (0,1);  |y|^2 = 1 everywhere;  rp = 0 except rp[0][2] = -4.5
    dist(n, m) = rp[n][m] - 2 x_n . y_m + |y_m|^2:
         n = 0:  -1   1  -1.5  1      ranking 2 0 1 3   (keys 1 and 3 tie exactly: smaller index first)
         n = 1:   1  -1   1   -1      ranking 1 3 0 2   (two exact ties)
         n = 2:   1   3   1    3      ranking 0 2 1 3"""
    x = np.array([[[1, 0, 0], [0, 1, -1]]], np.float32)                         # (1, 2, 3)
    y = np.array([[[1, 0, -1, 0], [0, 1, 0, 1]]], np.float32)                   # (1, 2, 4)
    rp = np.zeros((3, 4), np.float32)
    rp[0, 2] = -4.5
    xb, yb, sqy = H.prepared(x, y)
    assert torch.equal(xb, torch.from_numpy(x).double()) and torch.equal(yb, torch.from_numpy(y).double()) and bool((sqy == 1).all())
    D, topd, topi = H.reference(x, y, rp, 2, 2)
    assert D[0].tolist() == [[-1, 1, -1.5, 1], [1, -1, 1, -1], [1, 3, 1, 3]]
    assert topi[0].tolist() == [[2, 0, 1, 3], [1, 3, 0, 2], [0, 2, 1, 3]]
    assert topd[0].tolist() == [[-1.5, -1, 1, 1], [-1, -1, 1, 1], [1, 1, 3, 3]]
    E = H.bound(2, rp)
    assert E == 4 * 2.0 ** -24 * (4.5 + 3.1)
    want = torch.tensor([[[2, 1], [1, 0], [0, 1]]])                               # ranks 0 and 2
    assert H.judge(want, D, topd, topi, 2, 2, E) == (0.0, 0.0)
    assert H.judge(torch.tensor([[[2, 3], [1, 0], [0, 1]]]), D, topd, topi, 2, 2, E) == (1 / 6, 0.0)      # the tied key: tolerated
    with pytest.raises(AssertionError, match="beyond 2E"):
        H.judge(torch.tensor([[[2, 0], [1, 0], [0, 1]]]), D, topd, topi, 2, 2, E)


def test_a_subnormal_channel_does_not_reach_the_distance():
    """One query channel whose normalised value is an fp16 subnormal: the definition drops it, so two keys that differ only in the sign
    of that channel tie exactly — with the subnormal kept they would be 4 * 3e-5 * 0.5 apart."""
    x = np.array([[[1.0], [3e-5]]], np.float32)                                 # (1, 2, 1): th = (1, 3e-5) up to rounding
    y = np.array([[[0.5, 0.5], [0.5, -0.5]]], np.float32)                       # keys (0.5, 0.5) and (0.5, -0.5)
    xb, _, _ = H.prepared(x, y)
    assert xb[0, 1, 0] == 0.0 and xb[0, 0, 0] == 1.0
    D, _, topi = H.reference(x, y, None, 1, 2)
    assert D[0, 0, 0] == D[0, 0, 1] and topi[0, 0].tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------------------------ condition
@pytest.mark.parametrize("shape", R.FORMS, ids=R.shape_id)
def test_inputs_keep_near_ties_rare(shape):
    B, G, c, N, M_, k, d, bias = shape
    case = R.make_case(shape)
    _, topd, _ = H.reference(case["x"], case["y"], case["rp"], k, d, keep_D=False, values_only=True)
    share = H.near_tie_share(topd, H.bound(c, case["rp"]), k, d)
    print(f"near-tie share (fp16 definition) {R.shape_id(shape)}: {100 * share:.2f} %")
    assert share <= R.NEAR_TIE_CAP
