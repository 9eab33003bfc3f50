"""The max-relative aggregation's forward entry points through the C ABI, bit for bit against tests/mr_ref.py: gkg_mr_fwd_tm,
gkg_mr_fwd_tm16 (csrc/gkg_mr.hip mr_fwd_tm_kernel) and the channel-major gkg_mr_fwd (mr_fwd_kernel, mr_fwd_gather_kernel).  This
is where the two-launch form is pinned that test_hip_knn_mr_fused.py, test_hip_frozen_block_driver.py, test_hip_knn_prep_fused.py
and test_hip_knn_compact.py take as their baseline.  The aggregation is exact in fp32 — one subtraction, then a first maximum with
torch.max's NaN rule (reference torch_vertex.py:49-54) — so there is no tolerance anywhere in this file: m, the XM buffer and
argmax are compared as raw bits (NaN must be NaN where the reference is NaN; its payload is not compared).

Token-major shapes (B, G, c, N, M or self, k) = mr_ref.SHAPES_TM:
    (1, 1, 4, 1, self, 1)        everything degenerate (C = 4: mode 0 only)
    (3, 1, 16, 5, self, 1)       k = 1; B < 8: five of the eight XCD slots of the launch map return at once
    (9, 2, 8, 64, self, 9)       B = 9: a second round with seven padded images; N * C/4 = 256 exactly; the k = 9 instantiation
    (17, 4, 4, 65, 37, 9)        c = 4 (every thread its own k-NN group); 260 thread-columns: a second workgroup with four live
                                 threads; bipartite; three rounds
    (2, 2, 40, 51, 300, 5)       generic k; C/4 = 20, not a power of two (xm_col's multiply-high division); M > N
    (2, 3, 32, 50, self, 9)      G = 3: conv groups straddle k-NN groups
    (2, 4, 16, 63, self, 9), (2, 4, 16, 64, 90, 9)    N * C/4 = 1008 / 1024: a ragged and a full last workgroup
    (1, 2, 8, 40, 65536, 4)      lists naming rows 0 and 65535: the u16 limits of arg_kind 1 and of the compact lists
    (2, 1, 16, 30, 20, 255)      largest k (slot 254 in a u8); k > M: every list repeats
    (1, 8, 96, 33, self, 18)     C = 768, k = 18
Every shape runs in the three kinds of mr_ref.make_case ('ties': values on a grid, maxima tie; 'normal': with out-of-range list
entries, whose expectation is the clamped one; 'nonfinite': NaN in x / in src, +-inf, inf - inf, an all -inf list) and in the
cross product the entry point accepts: int64 / u16 lists, out_dtype F32 / BF16, mode 0 / 1 (C % 16 == 0), arg_kind 0 / 1 / no
argmax, and x given plain, with a row pitch of C + 8 (padding NaN, untouched), as the x half of a separate XM buffer and — mode 1,
F32 — as the x half of `out` itself, where only the m chunks may be written.

Channel-major shapes (BG, c, N, M or self, k) = mr_ref.SHAPES_CM, in F32, BF16 and F16 (inputs rounded first), argmax present / NULL:
    (1, 1, 1, self, 1)           everything degenerate
    (2, 5, 255 / 256 / 257, 37, 9)   one thread short of a query tile, exactly one, one past
    (3, 7, 70, self, 5)          c = 7: a channel block that is not a multiple of 4
    (1, 3, 40, 30000, 9)         a source row beyond the LDS budget: mr_fwd_gather_kernel
    (2, 70, 33, 50, 3)           c > 64: several channel chunks after the halving loop of the launch

Every output sits between guard bands (util.Buf), pre-filled with NaN / 0xFF; every call asserts the bands untouched."""
import numpy as np
import pytest
import torch

import mr_ref as R
from util import Buf

pytestmark = pytest.mark.gpu

_cases, _wants = {}, {}


def _L():
    from gkgnet_amd import _lib
    return _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    from gkgnet_amd.ops import _stream
    return _stream()


def _case(shape, kind):
    if (shape, kind) not in _cases:
        _cases[(shape, kind)] = R.make_case(shape, kind)
    return _cases[(shape, kind)]


def _want_tm(shape, kind, lists):
    """The token-major expectation, computed once per (case, list type) and never modified."""
    if (shape, kind, lists) not in _wants:
        _wants[(shape, kind, lists)] = R.expect_tm(_case(shape, kind), lists)
    return _wants[(shape, kind, lists)]


def _dev_lists(a, u16):
    """(BG, N, k) lists on the device: int64, or u16 carried in an int16 tensor."""
    if u16:
        return torch.from_numpy(a.astype(np.uint16).view(np.int16)).cuda()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _torch_dtype(code):
    L = _L()
    return {L.F32: torch.float32, L.BF16: torch.bfloat16, L.F16: torch.float16}[code]


class Arg:
    """argmax between guard bands: arg_kind 0 -> u8 slots (0xFF), 1 -> u16 rows (0xFFFF, held in an int16 tensor)."""

    def __init__(self, shape, arg_kind):
        self.kind = arg_kind
        self.buf = Buf(shape, torch.uint8) if arg_kind == 0 else Buf(shape, torch.int16, fill=-1)

    def values(self):
        v = self.buf.cpu()
        return v.to(torch.int64) if self.kind == 0 else v.to(torch.int64) & 0xFFFF

    def untouched(self):
        return bool((self.buf.t == self.buf.fill).all())


def _x_views(xt, C, mode, f32):
    """(name, tensor holding x, ldx, xchunk) for x (T, C) on the device; 'alias' is built by the caller inside `out`."""
    T = xt.shape[0]
    yield "plain", xt, 0, 0
    xp = torch.full((T, C + 8), float("nan"), device="cuda")
    xp[:, :C] = xt
    yield "pitch", xp, C + 8, 0
    if C % 16 == 0:
        yield "xm-half", R.xm_pack(xt, torch.full_like(xt, float("nan"))).contiguous(), 2 * C, C // 4
        if mode == 1 and f32:
            yield "alias", None, 2 * C, C // 4


def _run_tm(shape, x_dev, src_dev, lists_dev, u16, out_dtype, mode, arg_kind, view, want):
    """One call of gkg_mr_fwd_tm / _tm16 with everything asserted; ``view`` from _x_views."""
    L = _L()
    B, G, c, N, M_, k = shape
    C, T, M = G * c, B * N, (N if M_ is None else M_)
    name, holder, ldx, xchunk = view
    dt = _torch_dtype(out_dtype)
    out = Buf((T, 2 * C) if mode == 1 else (B, N, C), dt)
    if name == "alias":
        out.t.copy_(R.xm_pack(x_dev, torch.full_like(x_dev, float("nan"))))
        holder = out.t
    before = holder.clone()
    arg = None if arg_kind is None else Arg((B, N, C), arg_kind)
    fn = L.load().gkg_mr_fwd_tm16 if u16 else L.load().gkg_mr_fwd_tm
    what = f"{fn.__name__} {name} dtype={out_dtype} mode={mode} arg_kind={arg_kind}"
    L.check(fn(_p(holder), ldx, xchunk, _p(src_dev), _p(lists_dev), _p(out.t), None if arg is None else _p(arg.buf.t),
               B, G, c, N, M, k, mode, out_dtype, arg_kind or 0, _st()), what)
    torch.cuda.synchronize()
    assert out.guards_ok() and (arg is None or arg.buf.guards_ok()), what + ": wrote outside its outputs"
    if name != "alias":                                   # x is an input: bits, padding columns and NaN-filled m chunks unchanged
        assert torch.equal(holder.view(torch.int32), before.view(torch.int32)), what + ": x view modified"
    got = out.cpu()
    if mode == 0:
        assert R.same_bits(got, want["m"].to(dt)), what + ": m"
    else:
        assert R.same_bits(got, R.xm_of(want["x"], want["m"]).to(dt)), what + ": XM"
        if name == "alias":                               # only the m chunks were written: the x chunks keep their very bits
            xb, _ = R.xm_split(before.cpu())
            xa, _ = R.xm_split(got)
            assert torch.equal(xa.contiguous().view(torch.int32), xb.contiguous().view(torch.int32)), what + ": x chunks rewritten"
    if arg is not None:
        assert torch.equal(arg.values(), want["slot"].to(torch.int64) if arg_kind == 0 else want["row"]), what + ": argmax"


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", R.SHAPES_TM, ids=R.shape_id)
def test_token_major_forward_equals_the_definition_bit_for_bit(shape, kind):
    L = _L()
    B, G, c, N, M_, k = shape
    C = G * c
    case = _case(shape, kind)
    x_dev = torch.from_numpy(R.to_tm(case["x"], B)).reshape(B * N, C).cuda()
    src_dev = None if case["src"] is None else torch.from_numpy(R.to_tm(case["src"], B)).cuda()
    calls = 0
    for lists in ("idx", "idx16"):
        if case[lists] is None:
            continue
        want = _want_tm(shape, kind, lists)
        lists_dev = _dev_lists(case[lists], lists == "idx16")
        for out_dtype in (L.F32, L.BF16):
            for mode in ((0, 1) if C % 16 == 0 else (0,)):
                for view in _x_views(x_dev, C, mode, out_dtype == L.F32):
                    for arg_kind in (0, 1, None):
                        _run_tm(shape, x_dev, src_dev, lists_dev, lists == "idx16", out_dtype, mode, arg_kind, view, want)
                        calls += 1
    assert calls >= (12 if C % 16 else 78)


# ------------------------------------------------------------------------------------------------------------------ channel-major
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.float16), ids=("f32", "bf16", "f16"))
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", R.SHAPES_CM, ids=R.shape_id)
def test_channel_major_forward_equals_the_definition_bit_for_bit(shape, kind, dtype):
    L = _L()
    BG, c, N, M, k, self_graph = R.dims(shape)
    case = _case(shape, kind)
    code = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}[dtype]
    x = R.to_dtype(case["x"], dtype)                                            # inputs rounded to the dtype first
    src = None if self_graph else R.to_dtype(case["src"], dtype)
    m, slot, _ = R.mr_fwd(x.float().numpy(), None if src is None else src.float().numpy(), case["idx"], M)
    want = R.to_dtype(m, dtype)
    x_dev, src_dev, idx_dev = x.cuda(), (None if src is None else src.cuda()), _dev_lists(case["idx"], False)
    for with_arg in (True, False):
        out, arg = Buf((BG, c, N), dtype), (Buf((BG, c, N), torch.uint8) if with_arg else None)
        L.check(L.load().gkg_mr_fwd(_p(x_dev), _p(src_dev), _p(idx_dev), _p(out.t), None if arg is None else _p(arg.t), BG, c, N, M, k,
                                    code, _st()), "gkg_mr_fwd")
        torch.cuda.synchronize()
        assert out.guards_ok() and (arg is None or arg.guards_ok()), "gkg_mr_fwd wrote outside its outputs"
        assert R.same_bits(out.cpu(), want), "m"
        if arg is not None:
            assert torch.equal(arg.cpu(), torch.from_numpy(slot)), "argmax"


# ------------------------------------------------------------------------------------------------------------------ M beyond u16
BIG = (1, 2, 8, 40, 65537, 4)


def test_m_65537_runs_with_slots_and_is_refused_with_u16_rows():
    L = _L()
    B, G, c, N, M, k = BIG
    C = G * c
    case = R.make_case(BIG, "normal")
    assert case["idx16"] is None
    idx = case["idx"].copy()
    idx[:, 0, :] = 65536                                                        # the row no u16 could name, as a sure winner
    m, slot, row = R.mr_fwd(case["x"], case["src"], idx, M)
    assert (row == 65536).any()
    x_dev = torch.from_numpy(R.to_tm(case["x"], B)).cuda()
    src_dev = torch.from_numpy(R.to_tm(case["src"], B)).cuda()
    idx_dev = _dev_lists(idx, False)
    out, arg = Buf((B, N, C)), Buf((B, N, C), torch.uint8)
    L.check(L.load().gkg_mr_fwd_tm(_p(x_dev), 0, 0, _p(src_dev), _p(idx_dev), _p(out.t), _p(arg.t), B, G, c, N, M, k, 0, L.F32, 0, _st()),
            "gkg_mr_fwd_tm")
    torch.cuda.synchronize()
    assert out.guards_ok() and arg.guards_ok()
    assert R.same_bits(out.cpu(), torch.from_numpy(R.to_tm(m, B))) and torch.equal(arg.cpu(), torch.from_numpy(R.to_tm(slot, B)))
    # arg_kind 1 and the compact lists cannot name row 65536: refused, nothing written
    idx16_dev = torch.zeros((B * G, N, k), dtype=torch.int16, device="cuda")
    for fn, lists_dev, ak in ((L.load().gkg_mr_fwd_tm, idx_dev, 1), (L.load().gkg_mr_fwd_tm16, idx16_dev, 0),
                              (L.load().gkg_mr_fwd_tm16, idx16_dev, 1)):
        out, a16 = Buf((B, N, C)), Arg((B, N, C), 1)
        rc = fn(_p(x_dev), 0, 0, _p(src_dev), _p(lists_dev), _p(out.t), _p(a16.buf.t), B, G, c, N, M, k, 0, L.F32, ak, _st())
        torch.cuda.synchronize()
        assert rc == L.ERR_UNSUPPORTED, (fn.__name__, ak, rc)
        assert bool(torch.isnan(out.full).all()) and a16.untouched() and a16.buf.guards_ok()


# ------------------------------------------------------------------------------------------------------------------ error returns
def test_rejected_calls_return_the_documented_code_and_write_nothing():
    L = _L()
    K = L._K
    SHAPE, NULL, UNSUP = K["ERR_SHAPE"], K["ERR_NULL"], K["ERR_UNSUPPORTED"]
    B, G, c, N, k = 2, 2, 8, 12, 3
    C = G * c                                                                   # 16: mode 1 is available
    x = torch.randn(B * N, 2 * C, device="cuda")                                # wide enough for every view below
    idx = torch.zeros((B * G, N, k), dtype=torch.int64, device="cuda")
    ok = dict(x=x, ldx=0, xchunk=0, src=None, idx=idx, out="out", arg="arg", B=B, G=G, c=c, N=N, M=N, k=k, mode=0, dtype=L.F32, ak=0)
    table = [
        ("arg_kind 2", dict(ak=2), SHAPE),
        ("mode 2", dict(mode=2), SHAPE),
        ("mode 1 with C % 16 != 0", dict(mode=1, G=1, c=24), SHAPE),
        ("c % 4 != 0", dict(c=6), SHAPE),
        ("k = 0", dict(k=0), SHAPE),
        ("k = 256", dict(k=256), SHAPE),
        ("out_dtype F16", dict(dtype=L.F16), UNSUP),
        ("ldx < C", dict(ldx=C - 4), SHAPE),
        ("ldx % 4 != 0", dict(ldx=C + 2), SHAPE),
        ("xchunk does not divide C", dict(ldx=2 * C, xchunk=12), SHAPE),
        ("xchunk > 0 with ldx < 2C", dict(ldx=2 * C - 4, xchunk=C // 4), SHAPE),
        ("self graph with M != N", dict(M=N + 3), SHAPE),
        ("NULL x", dict(x=None), NULL),
        ("NULL nn_idx", dict(idx=None), NULL),
        ("NULL out", dict(out=None), NULL),
        ("x aliasing out with BF16", dict(x="out", ldx=2 * C, xchunk=C // 4, mode=1, dtype=L.BF16), SHAPE),
    ]
    for fn, lists in ((L.load().gkg_mr_fwd_tm, idx), (L.load().gkg_mr_fwd_tm16, torch.zeros((B * G, N, k), dtype=torch.int16, device="cuda"))):
        for what, change, code in table:
            a = dict(ok, idx=lists)
            a.update(change)
            out, arg = Buf((B * N, 2 * C)), Buf((B * N * C * 2,), torch.uint8)   # large enough for either mode and arg_kind
            ptr = lambda v: _p(out.t) if isinstance(v, str) and v == "out" else (_p(arg.t) if isinstance(v, str) else _p(v))  # noqa: E731
            rc = fn(ptr(a["x"]), a["ldx"], a["xchunk"], ptr(a["src"]), ptr(a["idx"]), ptr(a["out"]), ptr(a["arg"]), a["B"], a["G"],
                    a["c"], a["N"], a["M"], a["k"], a["mode"], a["dtype"], a["ak"], _st())
            torch.cuda.synchronize()
            assert rc == code, f"{fn.__name__}: {what}: returned {rc}, documented {code}"
            assert bool(torch.isnan(out.full).all()) and bool((arg.full == 255).all()), f"{fn.__name__}: {what}: outputs written"
            assert L.load().gkg_last_error_string() != b""
