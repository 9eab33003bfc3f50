"""tests/mr_ref.py's backward — the definition tests/test_hip_mr_bwd_abi.py holds the scatter kernels to — pinned on the CPU.

AGAINST THE ORACLE AND TORCH.  ``mr_ref.mr_bwd`` (fp64) rounded to fp32 gives the bits of oracle/c_oracle.mr_bwd on the 'integer'
kind (gradients i / 8: the oracle's fp32 chain is exact there) and equals torch.autograd of the literal max(x_j - x_i) formula in
fp64, with the in-range lists (neither of the two clamps the oracle and torch do not have).

EXACTNESS.  The GPU file demands the BITS of float32(definition) from every order-independent form.  That is fair only if the
fp64 sums of the definition are the exact sums: for every GPU case and kind the fp64 scatter is compared with an int64
fixed-point scatter of the same gradients (on the grid 2^-s the kind lives on).  A condition, not a measurement: 100 % of cases.

SENSITIVITY.  Eight wrong scatters are evaluated on the GPU tests' own inputs: each must differ from the definition, after
rounding to fp32, on EVERY case where the mistake can matter."""
import numpy as np
import pytest
import torch

import mr_ref as R

TM_SHAPES = sorted({v for s, _, _ in R.BWD_TM for v in R.bwd_variants(s)}, key=R.shape_id)
CM_SHAPES = sorted({v for s in R.SHAPES_CM for v in R.bwd_variants(s)}, key=R.shape_id)
CASES = [(s, kind) for s in TM_SHAPES for kind in R.BWD_KINDS] + [(s, kind) for s in CM_SHAPES for kind in ("integer", "normal")]
_cache = {}


def _case(shape, kind):
    if (shape, kind) not in _cache:
        _cache[(shape, kind)] = R.make_bwd_case(shape, kind)
    return _cache[(shape, kind)]


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return R.same_bits_z(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)))


def _tm(shape):
    return len(shape) == 6


def _combos(shape):
    """(arg kind, mode) the entry point of the shape accepts."""
    if not _tm(shape):
        return [(0, 0)]
    C = shape[1] * shape[2]
    return [(ak, mode) for ak in (0, 1) for mode in ((0, 1) if C % 16 == 0 else (0,))]


# ------------------------------------------------------------------------------------------------------------------ pinning
@pytest.mark.parametrize("shape", R.SHAPES_CM + R.SHAPES_TM, ids=R.shape_id)
def test_definition_equals_the_oracle_bit_for_bit_on_exact_gradients(shape):
    from oracle import c_oracle as O
    k = R.make_bwd_case(shape, "integer")
    res, (gx, gsrc) = R.bwd_expect(k, 0, 0, in_range=True)
    ox, os_ = O.mr_bwd(k["g"], k["base"], k["slot_in"], None if k["self"] else k["M"])
    assert _same(gx, ox) and _same(gsrc, os_)
    assert np.array_equal(res["gx"], ox) and (k["self"] or np.array_equal(res["gsrc"], os_))   # fp64 -> fp32: no rounding on this kind
    assert float(res["sabs"].max()) * 8 < 2 ** 24


@pytest.mark.parametrize("shape", [s for s in R.SHAPES_CM + R.SHAPES_TM if R.dims(s)[3] <= 512], ids=R.shape_id)
def test_definition_equals_autograd_of_the_literal_formula(shape):
    BG, c, N, M, kk, self_graph = R.dims(shape)
    k = R.make_bwd_case(shape, "integer")
    gen = torch.Generator().manual_seed(N + M)
    x = torch.randn(BG, c, N, dtype=torch.float64, generator=gen, requires_grad=True)
    src = None if self_graph else torch.randn(BG, c, M, dtype=torch.float64, generator=gen, requires_grad=True)
    s = x if self_graph else src
    j = torch.from_numpy(k["base"]).reshape(BG, 1, N * kk).expand(BG, c, N * kk)
    m, slot = torch.max(s.gather(2, j).reshape(BG, c, N, kk) - x.unsqueeze(-1), -1)              # torch_vertex.py:49-54
    m.backward(torch.from_numpy(k["g"]).double())
    res = R.mr_bwd(k["g"], k["base"], slot.numpy().astype(np.uint8), M, self_graph)
    assert np.array_equal(res["gx"], x.grad.numpy())                                         # exact: sums of i / 8
    assert self_graph or np.array_equal(res["gsrc"], src.grad.numpy())


def test_the_shape_list_reaches_every_form_by_the_restated_rule():
    seen = set()
    for s, flags, form in R.BWD_TM:
        B, G, c, N, M, _ = s
        got, cw, detail = R.bwd_form(B, G, c, N, M or N, flags)
        assert got == form, (R.bwd_id((s, flags, form)), got)
        seen.add((got, cw) + ((detail,) if got == "stream" else ()))
    for want in [("two-sweep", 4), ("two-sweep", 8), ("two-sweep", 16), ("stream-f64", 4), ("stream-f64", 8), ("stream-f64", 16),
                 ("private", 4), ("walk", 4), ("lds-f32", 4), ("lds-f32", 8), ("global-f32", None)]:
        assert want in seen, want
    streams = {t[1:] for t in seen if t[0] == "stream"}
    for cw in (4, 8, 16):                                                  # every chunk width, by rule and forced
        assert any(t[0] == cw for t in streams), cw
    for nt, u in ((512, 4), (512, 8), (256, 4), (256, 8)):                 # the four streaming instantiations
        assert any(t[1][:2] == (nt, u) for t in streams), (nt, u)
    assert any(t[1][2] for t in streams) and any(not t[1][2] for t in streams)      # exact and sampled scale
    # the boundaries, each side
    f = lambda *a: R.bwd_form(*a)[0]                                       # noqa: E731
    assert (f(2, 1, 16, 159, 159, 0), f(2, 1, 16, 160, 160, 0)) == ("two-sweep", "stream")
    assert (f(1, 1, 8, 50, 512, 0), f(1, 1, 8, 50, 513, 0)) == ("two-sweep", "lds-f32")
    assert (f(1, 1, 4, 160, 3071, 0), f(1, 1, 4, 160, 3072, 0)) == ("stream", "lds-f32")
    assert (f(1, 1, 4, 50, 3071, R.MR_DET), f(2, 1, 8, 50, 3072, R.MR_DET)) == ("two-sweep", "private")
    assert (f(1, 1, 4, 50, 6144, R.MR_F32), f(1, 1, 4, 50, 6145, R.MR_F32)) == ("lds-f32", "global-f32")
    assert (f(1, 1, 4, 70, 9216, R.MR_DET), f(2, 2, 4, 20, 9217, R.MR_DET)) == ("private", "walk")


# ------------------------------------------------------------------------------------------------------------------ exactness
EXACT = [(s, kind) for s, kind in CASES if kind != "normal"]            # 'normal' is held to the summation bound, not to bits


@pytest.mark.parametrize("shape,kind", EXACT, ids=[R.shape_id(s) + "-" + kind for s, kind in EXACT])
def test_the_fp64_sums_of_the_definition_are_the_exact_sums(shape, kind):
    k = _case(shape, kind)
    BG, c, N, M, kk, self_graph = R.dims(shape)
    assert N <= 4095                                       # SHMAX = 38 - bits(N) >= 26 (see the GPU file's docstring)
    s = R.exact_scale(kind)
    clean = np.ones((BG, c), bool)
    if k["dirty"]:
        clean[k["dirty"]] = False
    gi = np.where(clean[:, :, None], np.ldexp(k["g"].astype(np.float64), s), 0.0)
    assert np.array_equal(gi, np.rint(gi)) and float(np.abs(gi).max()) < 2 ** 32
    gi = gi.astype(np.int64)
    for ak, mode in _combos(shape):
        res, _ = R.bwd_expect(k, ak, mode)
        exact = np.zeros(BG * c * M, np.int64)
        np.add.at(exact, (np.arange(BG * c).reshape(BG, c, 1) * M + res["row"]).ravel(), gi.ravel())
        got = np.ldexp(res["scat"], s).reshape(BG * c, M)[clean.ravel()]
        assert np.array_equal(got, exact.reshape(BG * c, M)[clean.ravel()].astype(np.float64)), (ak, mode)
        assert int(np.abs(exact).max()) < 2 ** 50                                        # the total's pass through a double is exact
        if kind == "integer":                                                            # any fp32 order is exact: |partial| * 8 < 2^24
            assert float(res["sabs"].max()) * 8 < 2 ** 24
        if kind == "tiny":
            assert (k["g"] > 0).all() and (k["g"] < 2.0 ** -126).any() and (k["g"] >= 2.0 ** -126).any()


def test_generator_places_out_of_range_data_and_non_finite_values():
    for shape, kind in CASES:
        k = _case(shape, kind)
        BG, c, N, M, kk, _ = R.dims(shape)
        assert ((k["base"] >= 0) & (k["base"] < M)).all() and (k["slot_in"] < kk).all() and (k["row16_in"].astype(np.int64) < M).all()
        assert len(k["oor"]) >= 1 and sorted(int(k["idx"][p]) for p in k["oor"]) == sorted(R.oor_entries(M)[:len(k["oor"])])
        for b, n, j in k["oor"]:
            assert k["slot"][b, 0, n] == j and k["g"][b, 0, n] != 0
        if BG * N >= 9:
            assert len(k["oor"]) == 5 and [int(k["slot"][p]) for p in k["oor_slot"]] == [255, kk]
            assert [int(k["row16"][p]) for p in k["oor16"]] == R.bwd_oor16(M)
        if kind == "nonfinite" and N >= 8 and M >= 4:
            bg, ch = k["dirty"]
            col = R.bwd_expect(k, 0, 0)[0]["scat"][bg, ch]
            assert np.isposinf(col[1]) and np.isnan(col[2]) and np.isnan(col[3])
            assert np.isfinite(np.delete(k["g"].reshape(BG * c, N), bg * c + ch, axis=0)).all()
        if M == 65536:
            for ak in (0, 1):
                row = R.bwd_expect(k, ak, 0)[0]["row"]
                assert (row == 0).any() and (row == 65535).any()


# ------------------------------------------------------------------------------------------------------------------ wrong variants
def _lists(k, ak):
    return (k["row16"], None) if ak == 1 else (k["idx"], k["slot"])


def _differs(k, ak, mode, g=None, lists=None, **kw):
    """A wrong scatter of the case against the definition, both rounded to fp32."""
    want = R.bwd_expect(k, ak, mode)[0]
    a, s = _lists(k, ak)
    d = k["direct"] if mode == 1 else None
    got = R.mr_bwd(k["g"] if g is None else g, a if lists is None else lists, s, k["M"], k["self"], d, **kw)
    return not (_same(got["gx"], want["gx"]) and _same(got["gsrc"], want["gsrc"]))


_wrap = dict(rows=lambda i, M: np.mod(i, M), rows16=lambda r, M: np.mod(np.asarray(r).astype(np.int64), M))
_sext = dict(rows16=lambda r, M: R.clamp(np.asarray(r).astype(np.uint16).view(np.int16).astype(np.int64), M))


def _group0(k, ak, mode):
    G = k["shape"][1]
    return _differs(k, ak, mode, lists=k["idx"][(np.arange(k["idx"].shape[0]) // G) * G])


# (what, variant(k, ak, mode) -> differs, applies(k, dims, ak, mode))
VARIANTS = [
    ("row not clamped (wrapped modulo M)", lambda k, ak, mode: _differs(k, ak, mode, **_wrap),
     lambda k, d, ak, mode: d[3] > 8 and bool(k["oor16"] if ak else k["oor"]) and (not ak or d[3] + 7 < 65535)),
    ("slot not clamped to k - 1", lambda k, ak, mode: _differs(k, ak, mode, slots=lambda s, kk: np.asarray(s).astype(np.int64)),
     lambda k, d, ak, mode: ak == 0 and len(k["oor_slot"]) == 2 and d[3] > 8),
    ("seed direct + g", lambda k, ak, mode: _differs(k, ak, mode, seed=lambda d, g: d + g), lambda k, d, ak, mode: True),
    ("self-graph seed dropped", lambda k, ak, mode: _differs(k, ak, mode, keep_seed=False), lambda k, d, ak, mode: d[5]),
    ("last query row dropped", lambda k, ak, mode: _differs(k, ak, mode, n_used=d_n(k) - 1), lambda k, d, ak, mode: True),
    ("group index ch / C", _group0, lambda k, d, ak, mode: ak == 0 and _tm(k["shape"]) and k["shape"][1] > 1 and d[3] > 1),
    ("mode-1 gm column without the chunk offset", lambda k, ak, mode: _differs(k, ak, mode, g=k["direct"]),
     lambda k, d, ak, mode: mode == 1),
    ("u16 row sign-extended", lambda k, ak, mode: _differs(k, ak, mode, **_sext),
     lambda k, d, ak, mode: ak == 1 and d[3] > 1 and bool((k["row16"] >= 32768).any())),
]


def d_n(k):
    return k["g"].shape[2]


@pytest.mark.parametrize("what,variant,applies", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_wrong_variant_differs_on_every_applicable_case(what, variant, applies):
    hit = 0
    for shape, kind in CASES:
        k = _case(shape, kind)
        for ak, mode in _combos(shape):
            if not applies(k, R.dims(shape), ak, mode):
                continue
            assert variant(k, ak, mode), f"'{what}' is indistinguishable from the definition on {R.shape_id(shape)}-{kind} ak={ak} mode={mode}"
            hit += 1
    print(f"{what}: differs on all {hit} applicable cases")
    assert hit >= 8
