"""tests/mr_ref.py — the exact reference the GPU tests hold the max-relative forward kernels to — pinned on the CPU.

AGAINST THE ORACLE AND TORCH.  ``mr_ref.mr_fwd`` gives the bits of oracle/c_oracle.mr_fwd (m and the slot) and of the literal
reference formula torch.max(x_j - x_i, -1) (torch_vertex.py:49-54; NaN positions, bits elsewhere) on every channel-major case of
kinds 'ties' and 'nonfinite', with the in-range neighbour lists (neither of the two clamps).

SENSITIVITY.  Ten wrong implementations are evaluated on the GPU tests' own inputs: each must differ from the reference in at
least one element of (m, slot, row) — or of the rounded / packed output it concerns — on EVERY shape and kind where the mistake
can matter, or a kernel making it would pass tests/test_hip_mr_fwd_exact.py there.

GENERATOR.  Every shape with N >= 64 carries all five non-finite injections, every case of kinds 'normal' / 'nonfinite' its
out-of-range entries."""
import numpy as np
import pytest
import torch

import mr_ref as R

ALL = R.SHAPES_CM + R.SHAPES_TM
CASES = [(s, kind) for s in ALL for kind in R.KINDS]
IDS = [R.shape_id(s) + "-" + kind for s, kind in CASES]
_cache = {}


def _case(shape, kind):
    """(case, (m, slot, row) of the reference over the int64 lists); shared, never modified."""
    if (shape, kind) not in _cache:
        k = R.make_case(shape, kind)
        _cache[(shape, kind)] = (k, R.mr_fwd(k["x"], k["src"], k["idx"], k["M"]))
    return _cache[(shape, kind)]


def _same(a, b):
    """Bit equality of two fp32 arrays, NaN matching NaN."""
    return R.same_bits(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def _differs(got, want):
    return not (_same(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]))


# ------------------------------------------------------------------------------------------------------------------ pinning
@pytest.mark.parametrize("shape", R.SHAPES_CM, ids=R.shape_id)
@pytest.mark.parametrize("kind", ("ties", "nonfinite"))
def test_reference_equals_the_oracle_and_the_literal_formula(shape, kind):
    from oracle import c_oracle as O
    k = R.make_case(shape, kind)
    m, slot, row = R.mr_fwd(k["x"], k["src"], k["base"], k["M"])
    om, oslot = O.mr_fwd(k["x"], k["src"], k["base"])
    assert _same(m, om) and np.array_equal(slot, oslot)
    assert np.array_equal(row, np.take_along_axis(np.broadcast_to(k["base"][:, None], row.shape + (k["base"].shape[2],)),
                                                  slot[..., None].astype(np.int64), axis=3)[..., 0])
    x = torch.from_numpy(k["x"])
    s = x if k["src"] is None else torch.from_numpy(k["src"])
    BG, c, N = x.shape
    kk = k["base"].shape[2]
    j = torch.from_numpy(k["base"]).reshape(BG, 1, N * kk).expand(BG, c, N * kk)
    want = torch.max(s.gather(2, j).reshape(BG, c, N, kk) - x.unsqueeze(-1), -1).values
    assert R.same_bits(torch.from_numpy(m), want)
    if kind == "nonfinite" and N >= 64:
        assert np.isnan(m).any() and np.isposinf(m).any() and np.isneginf(m).any()


def test_generator_injects_everything_where_there_is_room():
    for s in ALL:
        BG, c, N, M, kk, _ = R.dims(s)
        k = R.make_case(s, "nonfinite")
        if N >= 64:
            assert tuple(k["injected"]) == R.INJECTIONS, (s, k["injected"])
        for kind in ("normal", "nonfinite"):
            k = R.make_case(s, kind)
            want = min(5, BG * N * kk)
            assert len(k["oor"]) == want and sorted(int(k["idx"][p]) for p in k["oor"]) == sorted(R.oor_entries(M)[:want]), s
            assert ((k["base"] >= 0) & (k["base"] < M)).all()
            if M < 65536 and BG * N * kk >= 7:
                assert [int(k["idx16"][p]) for p in k["oor16"]] == R.oor_entries(M, u16=True) and 65535 in k["idx16"]
            if k["idx16"] is not None:
                assert k["idx16"].min() >= 0 and k["idx16"].max() <= 65535
        if M == 65536:
            row = R.mr_fwd(k["x"], k["src"], k["idx16"], M)[2]
            assert (row == 0).any() and (row == 65535).any()
        assert not R.make_case(s, "ties")["oor"]


# ------------------------------------------------------------------------------------------------------------------ wrong variants
def _last_max(k, ref):
    return _differs(R.mr_fwd(k["x"], k["src"], k["idx"], k["M"], take=lambda v, b: (v >= b) | (np.isnan(v) & ~np.isnan(b))), ref)


def _fmaxf(k, ref):
    return _differs(R.mr_fwd(k["x"], k["src"], k["idx"], k["M"], take=lambda v, b: (v > b) | (np.isnan(b) & ~np.isnan(v))), ref)


def _xi_minus_xj(k, ref):
    return _differs(R.mr_fwd(k["x"], k["src"], k["idx"], k["M"], sub=lambda xj, xi: xi - xj), ref)


def _wrapped(k, ref):
    return _differs(R.mr_fwd(k["x"], k["src"], k["idx"], k["M"], rows=lambda i, M: np.mod(i, M)), ref)


def _truncated(k, ref):
    return _differs(R.mr_fwd(k["x"], k["src"], k["idx"], k["M"], rows=lambda i, M: R.clamp(i.astype(np.int32), M)), ref)


def _slot_for_row(k, ref):
    return not np.array_equal(ref[1].astype(np.int64), ref[2])


def _unclamped_row(k, ref):
    BG, c, N = ref[1].shape
    raw = np.take_along_axis(np.broadcast_to(k["idx"][:, None], (BG, c, N, k["idx"].shape[2])),
                             ref[1][..., None].astype(np.int64), axis=3)[..., 0]
    return not np.array_equal((raw & 0xFFFF).astype(np.uint16), ref[2].astype(np.uint16))


def _bf16_truncated(k, ref):
    m = torch.from_numpy(ref[0])
    want = m.bfloat16()
    got = (m.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)
    ok = ~torch.isnan(want)
    return not torch.equal(R.bits(got)[ok], R.bits(want)[ok])


def _xm_channel_interleaved(k, ref):
    B = k["shape"][0]
    x, m = torch.from_numpy(R.to_tm(k["x"], B)), torch.from_numpy(R.to_tm(ref[0], B))
    return not R.same_bits(torch.stack([x, m], dim=-1).reshape(-1, 2 * x.shape[-1]), R.xm_of(x, m))


def _group_by_conv_group(k, ref):
    """k-NN group of a channel taken as ch / (C / 4) (the conv group) instead of ch / c; list rows beyond the image's wrap."""
    B, G = k["shape"][:2]
    x4 = R.from_tm(R.to_tm(k["x"], B), 4)
    s4 = None if k["src"] is None else R.from_tm(R.to_tm(k["src"], B), 4)
    lists = np.stack([k["idx"][(b * G + q) % (B * G)] for b in range(B) for q in range(4)])
    m = R.to_tm(R.mr_fwd(x4, s4, lists, k["M"])[0], B)
    return not _same(m, R.to_tm(ref[0], B))


def _tm(k):
    return len(k["shape"]) == 6


# (what, the variant, the cases on which it must show)
VARIANTS = [
    ("last maximum wins", _last_max, lambda k, d: d[4] > 1),
    ("fmaxf semantics (a NaN is ignored)", _fmaxf, lambda k, d: "nan_src" in k["injected"]),
    ("x_i - x_j", _xi_minus_xj, lambda k, d: not (d[5] and d[2] == 1)),
    ("index wrapped modulo M", _wrapped, lambda k, d: bool(k["oor"]) and d[3] > 8),
    ("index truncated to int32 before the clamp", _truncated, lambda k, d: len(k["oor"]) == 5 and d[3] > 4),
    ("slot stored for the row / row for the slot", _slot_for_row, lambda k, d: d[3] > 1),
    ("unclamped row stored for arg_kind 1", _unclamped_row, lambda k, d: bool(k["oor"]) and d[3] > 1),
    ("bf16 by truncation", _bf16_truncated, lambda k, d: k["kind"] != "ties" and not (d[5] and d[2] == 1)),
    ("XM interleaved per channel", _xm_channel_interleaved, lambda k, d: _tm(k) and (k["shape"][1] * k["shape"][2]) % 16 == 0),
    ("group index ch / (C / 4)", _group_by_conv_group, lambda k, d: _tm(k) and k["shape"][1] != 4 and k["shape"][0] * k["shape"][1] > 1
     and d[4] < d[3]),                       # k >= M: lists may name every row, and m no longer depends on the list
]


@pytest.mark.parametrize("what,variant,applies", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_wrong_variant_differs_on_every_applicable_case(what, variant, applies):
    hit = 0
    for shape, kind in CASES:
        k, ref = _case(shape, kind)
        if not applies(k, R.dims(shape)):
            continue
        assert variant(k, ref), f"'{what}' is indistinguishable from the reference on {R.shape_id(shape)}-{kind}"
        hit += 1
    print(f"{what}: differs on all {hit} applicable cases")
    assert hit >= 4
