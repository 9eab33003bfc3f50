"""The max-relative aggregation's backward entry points through the C ABI — gkg_mr_bwd_tm, gkg_mr_bwd_tm_bnstats and the channel-major
gkg_mr_bwd (csrc/gkg_mr.hip) — against the fp64 definition tests/mr_ref.py::mr_bwd, in EVERY scatter form mr_bwd_tm_plan chooses
among.  tests/test_mr_bwd_reference_host.py pins that definition on the CPU and proves, per case, that its fp64 sums are the exact
sums; this file then asks for

  bits      of float32(definition) (mr_ref.bwd_bits; the sign of a zero is not compared) from every form on the 'integer' kind
            (gradients i / 8, |i| <= 64: every partial sum in any order is exact in fp32, atomics included), and from the
            fixed-point forms and the fp64-atomic variant on 'binades' (|g| in [2^-4, 2^4)) and 'tiny' ([2^-130, 2^-118), some
            addends subnormal).  Why the fixed-point forms owe bits there, N <= 4095: no addend is truncated (8 binades of spread
            + 6 of streaming headroom <= SHMAX = 38 - bits(N) >= 26), and the integer total spans at most 24 + 8 + 6 + 12 = 50
            bits, so its pass through a double is exact — gsrc == float32(sum), and the self graph's gx == float32(sum) +
            (direct - g) with the last two operations in fp32;
  the bound |got - want| <= fan_in * 2^-24 * sum|addend| + 2 * 2^-24 * |want| (mr_ref.sum_bound: any fp32 summation order plus the
            seed, derived, not measured) from the fp32-atomic forms, the private-accumulator form and the ordered walk;
  repeats   identical bits between the two runs every call gets, in every form but the fp32-atomic ones;
  'nonfinite' ('binades' with +inf, NaN and a +inf / -inf pair in one (image, channel)): NaN exactly where the IEEE sum is NaN,
            the right infinity where it is infinite, the bound on the rest of the chunk that fell back to fp32 atomics, bits in
            every other chunk.

Every case carries out-of-range data where the call reads it — int64 list entries, u16 rows >= M, slots >= k — whose expectation
is the clamped one (mr_targets / mr_bwd_kernel / mr_bwd_atomic_kernel clamp at every call site); every output lies between
NaN-filled guard bands; the form each case reaches is asserted from the dispatch rule restated in mr_ref.bwd_form.  'tiny' goes
to the fixed-point forms and the fp64-atomic variant only (fp32 atomic units need not keep subnormal addends).

Token-major cases: mr_ref.BWD_TM (shape, flags, form) — the two-sweep form at every SHAPES_TM entry of up to 512 keys and both
sides of N = 159 / 160 and M = 512 / 513; the four streaming instantiations by rule and forced, exact and sampled scale, chunk
widths 4 / 8 / 16, M = 3071 / 3072; GKG_MR_DETERMINISTIC at M = 3071 (still two-sweep), 3072 and 9216 (private accumulators,
TL = 3 / 1), 9217 and 65536 (ordered walk); fp32 atomics in LDS (M <= 6144) and global (6145, 65536).  A self-graph shape also
runs as a bipartite graph over M = N keys; every shape runs mode 0 and (C % 16 == 0) mode 1, arg_kind 0, 1 and 1 with nn_idx NULL."""
import functools

import numpy as np
import pytest
import torch

import mr_ref as R
from util import Buf

pytestmark = pytest.mark.gpu

ENTRIES = [(v, flags, form) for s, flags, form in R.BWD_TM for v in R.bwd_variants(s)]
RATIO = {}                                                   # form -> largest observed |error| / bound (printed per test)


def _L():
    from gkgnet_amd import _lib
    return _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    from gkgnet_amd.ops import _stream
    return _stream()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=16)
def _case(shape, kind):
    return R.make_bwd_case(shape, kind)


@functools.lru_cache(maxsize=16)
def _want(shape, kind, ak, mode):
    """The expectation of one (case, arg kind, mode), computed once and never modified."""
    return R.bwd_expect(_case(shape, kind), ak, mode)


@functools.lru_cache(maxsize=8)
def _inputs_tm(shape, kind):
    """Device inputs of a token-major case: gin per mode, the int64 lists, the u8 slots and the u16 rows (in an int16 tensor)."""
    B, G, c = shape[:3]
    C = G * c
    k = _case(shape, kind)
    g, d = torch.from_numpy(R.to_tm(k["g"], B)), torch.from_numpy(R.to_tm(k["direct"], B))
    gin = {0: g.cuda()}
    if C % 16 == 0:
        gin[1] = R.xm_pack(d.reshape(-1, C), g.reshape(-1, C)).contiguous().cuda()
    return dict(gin=gin, idx=_dev(k["idx"]), slot=_dev(R.to_tm(k["slot"], B)), row16=_dev(R.to_tm(k["row16"], B).view(np.int16)))


def _tm(a, B):
    return None if a is None else torch.from_numpy(R.to_tm(a, B))


def _check_bound(got, want64, fan, sabs, mask, form, what):
    """got fp32 against the fp64 definition under mr_ref.sum_bound where ``mask``; non-finite expectations by class."""
    res = dict(fan=fan.numpy(), sabs=sabs.numpy())
    bound = torch.from_numpy(R.sum_bound(res, want64.numpy()))
    fin = torch.isfinite(want64) & mask
    err = (got.double() - want64).abs()
    assert bool((err[fin] <= bound[fin]).all()), f"{what}: beyond the summation bound by {float((err[fin] / bound[fin]).max()):.3g}x"
    pos = fin & (bound > 0)
    if bool(pos.any()):
        RATIO[form] = max(RATIO.get(form, 0.0), float((err[pos] / bound[pos]).max()))
    bad = ~torch.isfinite(want64) & mask
    assert torch.equal(torch.isnan(got)[bad], torch.isnan(want64)[bad]), what + ": NaN placement"
    inf = bad & torch.isinf(want64)
    assert torch.equal(got.double()[inf], want64[inf]), what + ": infinities"


def _call_tm(shape, flags, gin, idx, arg, ak, mode, what):
    """gkg_mr_bwd_tm twice, each between fresh guard bands -> [(gx, gsrc)] on the host."""
    L = _L()
    B, G, c, N, M_, k = shape
    C, M = G * c, (N if M_ is None else M_)
    outs = []
    for _ in range(2):
        gx, gs = Buf((B, N, C)), (None if M_ is None else Buf((B, M, C)))
        L.check(L.load().gkg_mr_bwd_tm(_p(gin), _p(idx), _p(arg), _p(gx.t), None if gs is None else _p(gs.t), B, G, c, N, M, k, mode, ak,
                                       flags, _st()), what)
        torch.cuda.synchronize()
        assert gx.guards_ok() and (gs is None or gs.guards_ok()), what + ": wrote outside its outputs"
        outs.append((gx.cpu(), None if gs is None else gs.cpu()))
    return outs


def _dirty_mask(case, shape, cw):
    """(B, 1, C) mask of the channel chunk that holds the non-finite injections (the chunk that falls back to fp32 atomics)."""
    B, G, c = shape[:3]
    m = torch.zeros((B, 1, G * c), dtype=torch.bool)
    if case["dirty"] is not None:
        bg, ch = case["dirty"]
        col = (bg % G) * c + ch
        w = cw or G * c
        m[bg // G, 0, (col // w) * w:(col // w + 1) * w] = True
    return m


def _kinds(form):
    return R.BWD_KINDS if form in R.FIXED_POINT + ("stream-f64",) else tuple(k for k in R.BWD_KINDS if k != "tiny")


TM_PARAMS = [(e, kind) for e in ENTRIES for kind in _kinds(e[2])]


@pytest.mark.parametrize("entry,kind", TM_PARAMS, ids=[R.bwd_id(e) + "-" + kind for e, kind in TM_PARAMS])
def test_token_major_backward_equals_the_definition_in_every_form(entry, kind):
    shape, flags, form = entry
    B, G, c, N, M_, k = shape
    C, M, self_graph = G * c, (N if M_ is None else M_), M_ is None
    got_form, cw, _ = R.bwd_form(B, G, c, N, M, flags)
    assert got_form == form                                              # the form this case is here for, by the restated rule
    case, inp = _case(shape, kind), _inputs_tm(shape, kind)
    exact = kind == "integer" or form in R.FIXED_POINT + ("stream-f64",)
    dirty = _dirty_mask(case, shape, cw)
    calls = 0
    for mode in sorted(inp["gin"]):
        for ak, lists in ((0, inp["idx"]), (1, inp["idx"]), (1, None)):
            what = f"gkg_mr_bwd_tm {form} mode={mode} arg_kind={ak}{'' if lists is not None else ' nn_idx=NULL'}"
            res, (gx32, gs32) = _want(shape, kind, ak, mode)
            runs = _call_tm(shape, flags, inp["gin"][mode], lists, inp["slot"] if ak == 0 else inp["row16"], ak, mode, what)
            calls += 1
            dst_dirty = dirty.expand(B, M, C)
            for gx, gs in runs:
                dst, dst32, dst64 = (gx, gx32, res["gx"]) if self_graph else (gs, gs32, res["gsrc"])
                if not self_graph:                                       # gx = direct - g: one fp32 operation, bits in every form
                    assert R.same_bits_z(gx, _tm(gx32, B)), what + ": gx"
                if exact:
                    clean = ~dst_dirty
                    assert R.same_bits_z(torch.where(clean, dst, torch.zeros(())), torch.where(clean, _tm(dst32, B), torch.zeros(()))), \
                        what + ": not the bits of float32(definition)"
                _check_bound(dst, _tm(dst64, B), _tm(res["fan"], B), _tm(res["sabs"], B),
                             dst_dirty if exact else torch.ones_like(dst_dirty), form, what)
            if form in R.REPEATABLE or kind == "integer":                # bits repeat (outside a chunk that fell back to fp32 atomics)
                for a, b in zip(runs[0], runs[1]):
                    if a is not None:
                        keep = ~dirty.expand_as(a) | torch.tensor(form not in R.FIXED_POINT)
                        assert R.same_bits(torch.where(keep, a, torch.zeros(())), torch.where(keep, b, torch.zeros(()))), what + ": run to run"
    assert calls == (6 if C % 16 == 0 else 3)
    print(f"largest error / bound so far: {RATIO}")


# ------------------------------------------------------------------------------------------------------------------ headroom
def test_streaming_form_beyond_its_headroom_carries_the_two_sweep_bits_self_graph_slots():
    """A gradient 2^30 above everything the strided sample and the first iteration saw raises the workgroup's flag: it discards its
    image and re-runs the exact two-sweep body — the bits of the forced two-sweep call on the same chunk width.  Self graph,
    arg_kind 0 (tests/test_hip_mr_bwd_exact.py holds the bipartite arg_kind 1 case)."""
    B, G, c, N, k = 2, 2, 16, 700, 3
    shape = (B, G, c, N, None, k)
    case = _case(shape, "binades")
    C = G * c
    g = (R.to_tm(case["g"], B) * np.float32(2.0 ** -10)).astype(np.float32)
    # CW 16: 128 row lanes; the sample reads rows 0, 2, .. 510, the first iteration rows 0 .. 511: row 699 is in neither
    assert R.bwd_form(B, G, c, N, N, R.SV_STREAM | R.cw_bits(16)) == ("stream", 16, (512, 4, False))
    g[1, 699, 3] = np.float32(2.0 ** 22)
    gin, idx, slot = _dev(g), _dev(case["idx"]), _dev(R.to_tm(case["slot"], B))
    two = _call_tm(shape, R.SV_TWO | R.cw_bits(16), gin, idx, slot, 0, 0, "two-sweep")
    for flags in (R.SV_STREAM | R.cw_bits(16), R.SV_STREAM | R.cw_bits(16) | R.NT256 | R.ROWS8):
        one = _call_tm(shape, flags, gin, idx, slot, 0, 0, f"stream {flags:#x}")
        for gx, _ in one:
            assert R.same_bits(gx, two[0][0])
    # and the two-sweep bits are the definition's wherever no addend lost bits: the image without the large value is all of that
    res = R.mr_bwd(R.from_tm(g, G), case["idx"], case["slot"], N, True)
    gx32, _ = R.bwd_bits(R.from_tm(g, G), None, res, True)
    assert R.same_bits_z(two[0][0][0], _tm(gx32, B)[0])
    assert torch.allclose(two[0][0].double(), _tm(res["gx"], B), rtol=1e-6, atol=2.0 ** 22 * 2.0 ** -28 * 8)   # truncation below 2^-SHMAX


# ------------------------------------------------------------------------------------------------------------------ channel-major
_UT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}          # unit roundoff of the output's one rounding
CM_SHAPES = [v for s in R.SHAPES_CM for v in R.bwd_variants(s)]


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.float16), ids=("f32", "bf16", "f16"))
@pytest.mark.parametrize("kind", ("integer", "normal"))
@pytest.mark.parametrize("shape", CM_SHAPES, ids=R.shape_id)
def test_channel_major_backward_equals_the_definition(shape, kind, dtype):
    """gkg_mr_bwd: fp32 LDS atomics (any summation order) for rows within the LDS budget, fp32 global atomics beyond (fp32 tensors
    only).  g is rounded to the dtype first; 'integer': the bits of the exact result rounded once to the dtype; 'normal': the
    summation bound plus that one rounding."""
    L = _L()
    BG, c, N, M, k, self_graph = R.dims(shape)
    code = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}[dtype]
    case = _case(shape, kind)
    g = R.to_dtype(case["g"], dtype)
    res = R.mr_bwd(g.float().numpy(), case["idx"], case["slot"], M, self_graph)
    gx32, gs32 = R.bwd_bits(g.float().numpy(), None, res, self_graph)
    g_dev, idx_dev, slot_dev = g.cuda(), _dev(case["idx"]), _dev(case["slot"])
    lds_form = (R.LDS_BUDGET - k * 256 * 4) // (M * 4) >= 1
    form = "cm-lds-f32" if lds_form else "cm-global-f32"
    runs = []
    for _ in range(2):
        gx, gs = Buf((BG, c, N), dtype), (None if self_graph else Buf((BG, c, M), dtype))
        rc = L.load().gkg_mr_bwd(_p(g_dev), _p(idx_dev), _p(slot_dev), _p(gx.t), None if gs is None else _p(gs.t), BG, c, N, M, k, code, _st())
        torch.cuda.synchronize()
        assert gx.guards_ok() and (gs is None or gs.guards_ok())
        if not lds_form and dtype != torch.float32:                     # the global-atomic fallback is fp32 only: refused, nothing written
            assert rc == L.ERR_UNSUPPORTED and bool(torch.isnan(gx.full).all()) and (gs is None or bool(torch.isnan(gs.full).all()))
            assert L.load().gkg_last_error_string() != b""
            return
        L.check(rc, "gkg_mr_bwd")
        runs.append((gx.cpu(), None if gs is None else gs.cpu()))
    for gx, gs in runs:
        dst, dst32, dst64 = (gx, gx32, res["gx"]) if self_graph else (gs, gs32, res["gsrc"])
        if not self_graph:
            assert R.same_bits_z(gx, (-g.float()).to(dtype)), "gx = -g"
        if kind == "integer":
            assert R.same_bits_z(dst, R.to_dtype(dst32, dtype)), "not the exact result rounded once to the dtype"
        want = torch.from_numpy(dst64)
        u = _UT[dtype]
        bound = torch.from_numpy(R.sum_bound(res, dst64)) * (1 + u) + u * want.abs() + (2.0 ** -25 if dtype == torch.float16 else 0.0)
        err = (dst.double() - want).abs()
        assert bool((err <= bound).all()), float((err / bound).max())
        if dtype == torch.float32 and bool((bound > 0).any()):
            RATIO[form] = max(RATIO.get(form, 0.0), float((err / bound)[bound > 0].max()))
    if kind == "integer":
        assert all(b is None or R.same_bits(a, b) for a, b in zip(*runs))
    print(f"largest error / bound so far: {RATIO}")


# ------------------------------------------------------------------------------------------------------------------ bnstats
STATS_SHAPES = [v for s in R.TWO_SWEEP_SHAPES + R.STREAM_SHAPES if (s[1] * s[2]) % 16 == 0 for v in R.bwd_variants(s)]
# (shape, mode, flags): what gkg_mr_bwd_tm_bnstats must refuse — long sweeps, forced forms, fp32 atomics, mode 0, M = 3072
STATS_REFUSED = [((1, 1, 16, 600, 513, 2), 1, 0), ((1, 2, 8, 2052, 513, 1), 1, 0), ((2, 1, 16, 160, None, 3), 1, R.SV_STREAM | R.cw_bits(16)),
                 ((2, 1, 16, 160, None, 3), 1, R.cw_bits(8)), ((2, 1, 16, 160, None, 3), 1, R.SV_TWO), ((2, 1, 16, 160, None, 3), 1, R.MR_F32),
                 ((2, 1, 16, 160, None, 3), 0, 0), ((2, 4, 16, 64, 90, 9), 0, 0), ((1, 1, 16, 160, 3072, 1), 1, 0),
                 ((1, 1, 16, 50, 3072, 2), 1, R.MR_DET)]
STATS_PARAMS = [(s, 1, 0) for s in STATS_SHAPES if R.bwd_stats_supported(*s[:4], s[4] or s[3], 1)] + STATS_REFUSED


@pytest.mark.parametrize("shape,mode,flags", STATS_PARAMS, ids=[f"{R.shape_id(s)}-mode{m}-{f:#x}" for s, m, f in STATS_PARAMS])
def test_scatter_with_bn_statistics_runs_where_it_says_and_writes_nothing_where_not(shape, mode, flags):
    from test_hip_bwd_pass_fusion import _close
    L = _L()
    lib = L.load()
    B, G, c, N, M_, k = shape
    C, M, self_graph, T = G * c, (N if M_ is None else M_), M_ is None, B * N
    supported = R.bwd_stats_supported(B, G, c, N, M, mode, flags)
    assert supported == ((shape, mode, flags) not in STATS_REFUSED)
    case, inp = _case(shape, "binades"), _inputs_tm(shape, "binades")
    gen = torch.Generator(device="cuda").manual_seed(T + C)
    y = torch.randn(T, C, device="cuda", generator=gen) * 1.5 + 0.3
    mean, invstd = y.mean(0).contiguous(), (1.0 / torch.sqrt(y.var(0, unbiased=False) + 1e-5)).contiguous()
    for ak in (0, 1):
        arg = inp["slot"] if ak == 0 else inp["row16"]
        what = f"gkg_mr_bwd_tm_bnstats arg_kind={ak}"
        assert lib.gkg_mr_bwd_tm_bnstats_supported(B, G, c, N, M, k, mode, ak, 1 if self_graph else 0, flags) == (1 if supported else 0), what
        gx, gs, sums = Buf((B, N, C)), (None if self_graph else Buf((B, M, C))), Buf((2, C), torch.float64, zero=True)
        rc = lib.gkg_mr_bwd_tm_bnstats(_p(inp["gin"][mode]), _p(inp["idx"]), _p(arg), _p(gx.t), None if gs is None else _p(gs.t), B, G, c, N,
                                       M, k, mode, ak, flags, _p(y), _p(mean), _p(invstd), _p(sums.t), _st())
        torch.cuda.synchronize()
        assert gx.guards_ok() and (gs is None or gs.guards_ok()) and sums.guards_ok(), what + ": wrote outside its outputs"
        assert (rc == 0) == supported, what
        if not supported:
            assert rc == L.ERR_UNSUPPORTED and lib.gkg_last_error_string() != b""
            assert bool(torch.isnan(gx.full).all()) and (gs is None or bool(torch.isnan(gs.full).all())) and bool((sums.t == 0).all())
            continue
        plain = _call_tm(shape, flags, inp["gin"][mode], inp["idx"], arg, ak, mode, "gkg_mr_bwd_tm")[0]
        assert R.same_bits(gx.cpu(), plain[0]) and (gs is None or R.same_bits(gs.cpu(), plain[1])), what + ": not the plain call's bits"
        g64 = gx.t.double().reshape(T, C)
        want = torch.stack([g64.sum(0), (g64 * ((y.double() - mean.double()) * invstd.double())).sum(0)])
        assert _close(sums.t, want), (what, float((sums.t - want).abs().max()), float(want.abs().max()))


# ------------------------------------------------------------------------------------------------------------------ error returns
def test_rejected_calls_return_the_documented_code_and_write_nothing():
    L = _L()
    lib, K = L.load(), L._K
    SHAPE, NULL, UNSUP = K["ERR_SHAPE"], K["ERR_NULL"], K["ERR_UNSUPPORTED"]
    B, G, c, N, k = 2, 2, 8, 12, 3
    C = G * c                                                                   # 16: mode 1 is available
    gin = torch.randn(B * N, 2 * C, device="cuda")                              # wide enough for either mode
    idx = torch.zeros((B * G, N, k), dtype=torch.int64, device="cuda")
    arg = torch.zeros((B, N, C), dtype=torch.int16, device="cuda")              # wide enough for either arg kind
    y, mean = torch.randn(B * N, C, device="cuda"), torch.zeros(C, device="cuda")

    def run(fn, a):
        gx, gs, sums = Buf((B * 40, C)), Buf((B * 40, C)), Buf((2, C), torch.float64, zero=True)
        ptr = {"gx": _p(gx.t), "gs": _p(gs.t), "sums": _p(sums.t), None: None}
        p = lambda v: ptr[v] if (v is None or isinstance(v, str)) else _p(v)    # noqa: E731
        if fn == "cm":
            rc = lib.gkg_mr_bwd(p(a["gin"]), p(a["idx"]), p(a["arg"]), p(a["gx"]), p(a["gs"]), a["B"] * a["G"], a["c"], a["N"], a["M"], a["k"],
                                a["dtype"], _st())
        elif fn == "tm":
            rc = lib.gkg_mr_bwd_tm(p(a["gin"]), p(a["idx"]), p(a["arg"]), p(a["gx"]), p(a["gs"]), a["B"], a["G"], a["c"], a["N"], a["M"], a["k"],
                                   a["mode"], a["ak"], a["flags"], _st())
        else:
            rc = lib.gkg_mr_bwd_tm_bnstats(p(a["gin"]), p(a["idx"]), p(a["arg"]), p(a["gx"]), p(a["gs"]), a["B"], a["G"], a["c"], a["N"], a["M"],
                                           a["k"], a["mode"], a["ak"], a["flags"], p(a["y"]), p(a["mean"]), p(a["invstd"]), p(a["sums"]), _st())
        torch.cuda.synchronize()
        written = not (bool(torch.isnan(gx.full).all()) and bool(torch.isnan(gs.full).all()) and bool((sums.t == 0).all()) and sums.guards_ok())
        return rc, written

    ok = dict(gin=gin, idx=idx, arg=arg, gx="gx", gs=None, B=B, G=G, c=c, N=N, M=N, k=k, mode=1, ak=0, flags=0, dtype=L.F32,
              y=y, mean=mean, invstd=mean, sums="sums")
    common = [
        ("NULL gin", dict(gin=None), NULL), ("NULL argmax", dict(arg=None), NULL), ("NULL gx", dict(gx=None), NULL),
        ("NULL nn_idx with arg_kind 0", dict(idx=None), NULL),
        ("N = 0", dict(N=0, M=0), SHAPE), ("M = 0", dict(M=0, gs="gs"), SHAPE), ("c = 0", dict(c=0), SHAPE), ("B = -1", dict(B=-1), SHAPE),
        ("k = 0", dict(k=0), SHAPE), ("k = 256", dict(k=256), SHAPE),
        ("self graph with M != N", dict(M=N + 3), SHAPE),
    ]
    tm_only = [
        ("c % 4 != 0", dict(c=6), SHAPE), ("G = 0", dict(G=0), SHAPE), ("mode 2", dict(mode=2), SHAPE),
        ("mode 1 with C % 16 != 0", dict(G=1, c=24), SHAPE), ("arg_kind 2", dict(ak=2), SHAPE),
    ]
    table = ([("cm", w, ch, code) for w, ch, code in common]
             + [("cm", "BG > 65535", dict(B=65536, G=1), UNSUP), ("cm", "unknown dtype", dict(dtype=77), UNSUP)]
             + [(fn, w, ch, code) for fn in ("tm", "bn") for w, ch, code in common + tm_only]
             + [("tm", "forced streaming width that does not fit", dict(M=20000, gs="gs", flags=R.SV_STREAM | R.cw_bits(16)), UNSUP),
                ("tm", "forced fp64-atomic width that does not divide c", dict(flags=R.SV_F64 | R.cw_bits(16)), UNSUP),
                ("bn", "NULL y", dict(y=None), NULL), ("bn", "NULL mean", dict(mean=None), NULL), ("bn", "NULL invstd", dict(invstd=None), NULL),
                ("bn", "NULL sums", dict(sums=None), NULL), ("bn", "mode 0", dict(mode=0), UNSUP),
                ("bn", "fp32 atomics", dict(flags=R.MR_F32), UNSUP), ("bn", "forced form", dict(flags=R.SV_TWO), UNSUP)])
    for fn, what, change, code in table:
        a = dict(ok)
        a.update(change)
        rc, written = run(fn, a)
        assert rc == code, f"{fn}: {what}: returned {rc}, documented {code}"
        assert not written, f"{fn}: {what}: outputs written"
        assert lib.gkg_last_error_string() != b"", f"{fn}: {what}: no error string"
    # the table's starting point is a valid call of each entry point, and nn_idx may be NULL with arg_kind 1
    for fn, change in (("cm", {}), ("tm", {}), ("bn", {}), ("tm", dict(idx=None, ak=1)), ("bn", dict(idx=None, ak=1))):
        a = dict(ok)
        a.update(change)
        rc, written = run(fn, a)
        assert rc == 0 and written, (fn, change, rc)
