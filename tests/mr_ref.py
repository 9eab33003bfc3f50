"""Plain numpy/torch restatement of the max-relative aggregation's forward (include/gkg_hip.h: gkg_mr_fwd, gkg_mr_fwd_tm,
gkg_mr_fwd_tm16 and the operand producer of gkg_mr_linear_bf16) and of its backward scatter (gkg_mr_bwd, gkg_mr_bwd_tm: the last
section of this file), and the inputs the tests hold the kernels to them with.

    m[bg][ch][n] = max_j ( src[bg][ch][clamp(idx[bg][n][j])] - x[bg][ch][n] )        (reference torch_vertex.py:49-54)

The operation is exact in fp32 (one subtraction, then a first-maximum with torch.max's NaN rule), so this file IS the expected
value, bit for bit: tests/test_hip_mr_fwd_exact.py compares raw bits, tests/test_mr_reference_host.py pins ``mr_fwd`` to the C
oracle and to the literal torch formula on the CPU and shows that each of a list of wrong formulas differs from it on these inputs.

The module also holds what the GPU files and the host file must share so that they cannot drift: the shape lists and the case
generator.  A helper module, not a test module and not a conftest; it imports nothing of the package and nothing of oracle/."""
import numpy as np
import torch

from util import xm_pack, xm_split                                            # noqa: F401  (re-exported: the XM layout)

# (B, G, c, N, M (None = self graph), k) — token-major entry points; see tests/test_hip_mr_fwd_exact.py for what each reaches
SHAPES_TM = [(1, 1, 4, 1, None, 1), (3, 1, 16, 5, None, 1), (9, 2, 8, 64, None, 9), (17, 4, 4, 65, 37, 9), (2, 2, 40, 51, 300, 5),
             (2, 3, 32, 50, None, 9), (2, 4, 16, 63, None, 9), (2, 4, 16, 64, 90, 9), (1, 2, 8, 40, 65536, 4), (2, 1, 16, 30, 20, 255),
             (1, 8, 96, 33, None, 18)]
# (BG, c, N, M (None = self graph), k) — channel-major gkg_mr_fwd
SHAPES_CM = [(1, 1, 1, None, 1), (2, 5, 255, 37, 9), (2, 5, 256, 37, 9), (2, 5, 257, 37, 9), (3, 7, 70, None, 5), (1, 3, 40, 30000, 9),
             (2, 70, 33, 50, 3)]
KINDS = ("ties", "normal", "nonfinite")
INJECTIONS = ("nan_x", "nan_src", "inf_src", "inf_minus_inf", "all_neg_inf")


def shape_id(s):
    return "x".join("self" if v is None else str(v) for v in s)


def dims(shape):
    """(BG, c, N, M, k, self_graph) of a SHAPES_TM or SHAPES_CM entry."""
    if len(shape) == 6:
        B, G, c, N, M, k = shape
        BG = B * G
    else:
        BG, c, N, M, k = shape
    return BG, c, N, (N if M is None else M), k, M is None


# ------------------------------------------------------------------------------------------------------------------ reference
def clamp(idx, M):
    """What every forward form does with a neighbour index: < 0 -> 0, >= M -> M - 1, decided on the full int64 value."""
    return np.clip(np.asarray(idx, dtype=np.int64), 0, M - 1)


def takes(v, best):
    """torch.max's running-maximum rule (torch_vertex.py:54): a larger value wins, the first of equals stays, a NaN replaces a
    non-NaN best and then stays."""
    return (v > best) | (np.isnan(v) & ~np.isnan(best))


def _gather(src, rows):
    """src (BG, c, M), rows (BG, N) -> (BG, c, N)."""
    BG, c, _ = src.shape
    return np.take_along_axis(src, np.broadcast_to(rows[:, None, :], (BG, c, rows.shape[1])), axis=2)


def mr_fwd(x, src, idx, M, sub=None, take=takes, rows=clamp):
    """x (BG, c, N) fp32, src (BG, c, M) fp32 or None (self graph), idx (BG, N, k) integers -> (m fp32, slot u8, row int64), each
    (BG, c, N): the maximum, the first j attaining it and the clamped index idx[n][slot].  ``sub`` / ``take`` / ``rows`` replace
    the subtraction, the running-maximum rule and the index rule (the host test's wrong variants)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    s = x if src is None else np.ascontiguousarray(src, dtype=np.float32)
    assert s.shape[2] == M
    ic = rows(idx, M)
    sub = sub or (lambda xj, xi: xj - xi)
    with np.errstate(invalid="ignore", over="ignore"):
        best = sub(_gather(s, ic[:, :, 0]), x).astype(np.float32)
        slot = np.zeros(x.shape, np.uint8)
        row = np.broadcast_to(ic[:, None, :, 0], x.shape).copy()
        for j in range(1, ic.shape[2]):
            v = sub(_gather(s, ic[:, :, j]), x).astype(np.float32)
            t = take(v, best)
            best = np.where(t, v, best)
            slot = np.where(t, np.uint8(j), slot)
            row = np.where(t, ic[:, None, :, j], row)
    return best, slot, row


def to_dtype(a, dtype):
    """fp32 array -> tensor of ``dtype`` by torch's conversion: round-to-nearest-even, NaN stays NaN, overflow goes to inf."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)


def bits(t):
    """Raw bits of a tensor as integers (uint8 tensors as they are)."""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.contiguous().view(torch.int16)
    return t


def same_bits(got, want):
    """True when two float tensors have NaN at the same places and identical bits everywhere else (signed zeros and infinities
    included; NaN payloads are not compared)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(bits(got)[~wn], bits(want)[~wn]))


# ------------------------------------------------------------------------------------------------------------------ token-major
def to_tm(a, B):
    """(B G, c, N) -> (B, N, C = G c): channel g c + ch of token n is group g's channel ch."""
    BG, c, N = a.shape
    return np.ascontiguousarray(a.reshape(B, (BG // B) * c, N).transpose(0, 2, 1))


def from_tm(a, G):
    """(B, N, C) -> (B G, C / G, N)."""
    B, N, C = a.shape
    return np.ascontiguousarray(a.transpose(0, 2, 1).reshape(B * G, C // G, N))


def xm_of(x_tm, m_tm):
    """x, m (B, N, C) tensors -> the XM operand buffer (B N, 2 C) of include/gkg_hip.h "XM layout"."""
    C = x_tm.shape[-1]
    return xm_pack(x_tm.reshape(-1, C), m_tm.reshape(-1, C))


def expect_tm(case, lists="idx"):
    """Token-major expectation of a SHAPES_TM case: dict of fp32 tensors x, m (B, N, C), slot u8 and row (int64, < M) (B, N, C).
    ``lists``: which of the case's neighbour lists the call reads ('idx' int64, 'idx16' u16, 'base' in range)."""
    B = case["shape"][0]
    m, slot, row = mr_fwd(case["x"], case["src"], case[lists], case["M"])
    t = lambda a: torch.from_numpy(to_tm(a, B))                                # noqa: E731
    return dict(x=t(case["x"]), m=t(m), slot=t(slot), row=t(row))


# ------------------------------------------------------------------------------------------------------------------ cases
BOOST = 6.0           # kinds 'normal' / 'nonfinite': added to source rows 0 and M - 1, the rows a clamped index lands on, so that a clamped entry
#                       wins its maximum (and a wrapped, truncated or unclamped index shows in m and in the stored row)
_Q_NAN, _Q_PINF, _Q_NINF, _Q_IMI, _Q_ALLN = (1, 2, 3), 4, 5, 6, 7      # queries the non-finite injections use
_R_NAN, _R_PINF, _R_NINF = 2, 3, 4                                    # source rows they use (bipartite; self graph: see below)
_Q_U16 = (10, 11, 12)                                                  # queries whose lists name rows 0 and M - 1 (M = 65536)


def oor_entries(M, u16=False):
    """The out-of-range entries of kinds 'normal' / 'nonfinite': int64 lists, or u16 lists (M < 65536 only)."""
    if not u16:
        return [-5, M + 7, 2 ** 32 + 3, -(2 ** 40), 2 ** 63 - 1]
    return ([M + 7] if M + 7 <= 65535 else []) + [65535] if M < 65536 else []


def make_case(shape, kind, seed=0):
    """-> dict: shape, M, self, x (BG, c, N) fp32, src (BG, c, M) fp32 or None, base (BG, N, k) int64 in-range lists, idx (base
    plus the int64 out-of-range entries), idx16 (base plus the u16 ones; None when M > 65536), oor / oor16 (their positions),
    injected (names of the non-finite injections made)."""
    assert kind in KINDS
    BG, c, N, M, k, self_graph = dims(shape)
    rng = np.random.default_rng([seed, KINDS.index(kind), BG, c, N, M, k])
    if kind == "ties":
        draw = lambda *s: (rng.integers(-8, 9, size=s) / 4.0).astype(np.float32)      # noqa: E731
    else:
        draw = lambda *s: rng.standard_normal(size=s).astype(np.float32)              # noqa: E731
    x = draw(BG, c, N)
    src = x if self_graph else draw(BG, c, M)
    base = rng.integers(0, M, size=(BG, N, k), dtype=np.int64)
    used = set()                                               # queries whose lists are arranged by hand below
    base[:, ::3, k - 1] = base[:, ::3, 0]                      # every third row repeats its first neighbour (in its last slot)
    if M == 65536 and N > max(_Q_U16) and k >= 2:              # the u16 limits, as winners (a list of one row) and side by side
        base[:, _Q_U16[0], :2] = (0, 65535)
        base[:, _Q_U16[1], :] = 65535
        base[:, _Q_U16[2], :] = 0
        used |= set(_Q_U16)
    injected = []
    if kind != "ties":
        src[:, :, 0] += BOOST
        src[:, :, M - 1] += BOOST
    if kind == "nonfinite":
        bg, room = BG - 1, N >= 8 and M >= 8 and k >= 2
        if N >= 2:                                             # a NaN in x: every difference of that (query, channel) is NaN
            x[0, c - 1, N - 1] = np.nan
            injected.append("nan_x")
            used.add(N - 1)
        if room:
            ch = (0, 1 % c, 2 % c)
            r_pinf = _Q_IMI if self_graph else _R_PINF         # self graph: the query that is +inf is its own +inf neighbour
            src[bg, ch[0], _R_NAN] = np.nan                    # a NaN source value listed at the first, a middle and the last slot
            for q, j in zip(_Q_NAN, (0, k // 2, k - 1)):
                base[bg, q, j] = _R_NAN
            injected.append("nan_src")
            src[bg, ch[1], r_pinf] = np.inf
            src[bg, ch[2], _R_NINF] = -np.inf
            base[bg, _Q_PINF, 1] = r_pinf
            base[bg, _Q_NINF, 0] = _R_NINF
            injected.append("inf_src")
            x[bg, ch[1], _Q_IMI] = np.inf                      # inf - inf
            base[bg, _Q_IMI, k - 1] = r_pinf
            injected.append("inf_minus_inf")
            base[bg, _Q_ALLN, :] = _R_NINF                     # every neighbour -inf in channel ch[2]
            injected.append("all_neg_inf")
            used |= set(_Q_NAN) | {_Q_PINF, _Q_NINF, _Q_IMI, _Q_ALLN}
    idx, idx16, oor, oor16 = base.copy(), (base.copy() if M <= 65536 else None), [], []
    if kind != "ties":
        free = [n for n in range(N) if n not in used] or list(range(N))
        slots = [(b, n, 0) for b in range(BG) for n in free]   # slot 0: the clamped entry wins ties against later repeats of its row
        if len(slots) < 7:
            slots = [(b, n, j) for b in range(BG) for n in free for j in range(k)]
        order = rng.permutation(len(slots))
        for i, e in enumerate(oor_entries(M)[:len(slots)]):
            idx[slots[order[i]]] = e
            oor.append(slots[order[i]])
        if idx16 is not None:
            for i, e in enumerate(oor_entries(M, u16=True)[:len(slots)]):
                idx16[slots[order[-1 - i]]] = e
                oor16.append(slots[order[-1 - i]])
    return dict(shape=shape, kind=kind, M=M, self=self_graph, x=x, src=None if self_graph else src, base=base, idx=idx, idx16=idx16,
                oor=oor, oor16=oor16, injected=injected)


# ------------------------------------------------------------------------------------------------------------------ backward
# The backward of the aggregation is a scatter (include/gkg_hip.h: gkg_mr_bwd, gkg_mr_bwd_tm):
#
#     row[bg][ch][n] = clamp(idx[bg][n][min(slot[bg][ch][n], k - 1)], M)      arg kind 0 (u8 winning slots + the int64 lists)
#                    = min(row16[bg][ch][n], M - 1)                           arg kind 1 (u16 winning rows; the lists are not read)
#     gx             = direct - g             (direct = 0 for mode 0 and for the channel-major call)
#     dst[bg][ch][row] += g[bg][ch][n]        dst = gsrc, or gx itself for the self graph
#
# ``mr_bwd`` evaluates it in fp64; tests/test_mr_bwd_reference_host.py pins it to the C oracle and to torch.autograd of the
# literal formula, proves per case that the fp64 sums ARE the exact sums (so "the bits of float32(definition)" is a fair demand
# of the order-independent kernels), and shows that each of a list of wrong scatters differs from it on these inputs.
BWD_KINDS = ("integer", "binades", "tiny", "nonfinite")      # + 'normal' (channel-major bound cases)
U24 = 2.0 ** -24                                             # unit roundoff of fp32
MR_DET, MR_F32 = 1, 2                                        # GKG_MR_DETERMINISTIC, GKG_MR_FP32_ATOMICS
SV_STREAM, SV_F64, SV_TWO = 1 << 16, 2 << 16, 3 << 16        # measurement bits 16..17: forced streaming / fp64-atomic / two-sweep
NT256, ROWS8 = 2 << 20, 1 << 22                              # bits 20..21 = 2: 256 threads; bit 22: 8 rows in flight
LDS_BUDGET = 96 * 1024


def cw_bits(cw):
    return cw << 8                                           # bits 8..15: forced chunk width


def slot_clamp(slot, k):
    return np.minimum(np.asarray(slot).astype(np.int64), k - 1)


def row16_clamp(row16, M):
    return np.minimum(np.asarray(row16).astype(np.int64) & 0xFFFF, M - 1)


def bwd_rows(idx_or_rows, slot, M, c=None, rows=clamp, slots=slot_clamp, rows16=row16_clamp):
    """Destination rows (BG, c, N), int64 in [0, M).  arg kind 0: idx_or_rows = lists (BG, N, k) int64, slot (BG, c, N) u8.  arg
    kind 1: slot is None and idx_or_rows = rows (BG, c, N) u16.  A slot rule that returns j >= k reads the list memory past the
    row, as an unclamped kernel would (wrapping at the end of the tensor); the correct rule never does."""
    if slot is None:
        return rows16(idx_or_rows, M)
    idx = np.ascontiguousarray(idx_or_rows, dtype=np.int64)
    BG, N, k = idx.shape
    s = slots(slot, k)
    pos = (np.arange(BG)[:, None, None] * N + np.arange(N)[None, None, :]) * k + s
    return rows(idx.reshape(-1)[pos % idx.size], M)


def mr_bwd(g, idx_or_rows, slot_or_None, M, self_graph, direct=None, rows=clamp, slots=slot_clamp, rows16=row16_clamp,
           seed=lambda d, g: d - g, keep_seed=True, n_used=None):
    """The definition, in fp64.  g, direct (BG, c, N) -> dict:
        gx (BG, c, N), gsrc (BG, c, M) or None (self graph)   the result
        scat (BG, c, M)   the scattered sums alone (== gsrc; the self graph's gx is seed + scat)
        fan, sabs         per element of the destination (gx for the self graph, gsrc otherwise): the number of addends and the
                          sum of their magnitudes — for the self graph the token's own seed direct - g counts as one addend
        row (BG, c, N)    the destination rows
    ``rows`` / ``slots`` / ``rows16`` / ``seed`` / ``keep_seed`` / ``n_used`` replace the row clamp, the slot clamp, the u16 row rule,
    the seed, drop the self graph's seed and limit the scatter to the first n_used queries (the host test's wrong variants)."""
    g64 = np.asarray(g, dtype=np.float64)
    BG, c, N = g64.shape
    row = bwd_rows(idx_or_rows, slot_or_None, M, c, rows, slots, rows16)
    assert row.shape == g64.shape and row.min() >= 0 and row.max() < M
    flat = (np.arange(BG * c).reshape(BG, c, 1) * M + row)
    nu = N if n_used is None else n_used
    fl, gv = flat[:, :, :nu].ravel(), g64[:, :, :nu].ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        scat = np.bincount(fl, weights=gv, minlength=BG * c * M).reshape(BG, c, M)
        sabs = np.bincount(fl, weights=np.abs(gv), minlength=BG * c * M).reshape(BG, c, M)
        fan = np.bincount(fl, minlength=BG * c * M).reshape(BG, c, M)
        sd = seed(np.zeros_like(g64) if direct is None else np.asarray(direct, dtype=np.float64), g64)
        if not self_graph:
            return dict(gx=sd, gsrc=scat, scat=scat, fan=fan, sabs=sabs, row=row)
        if not keep_seed:
            return dict(gx=scat.copy(), gsrc=None, scat=scat, fan=fan, sabs=sabs, row=row)
        return dict(gx=sd + scat, gsrc=None, scat=scat, fan=fan + 1, sabs=sabs + np.abs(sd), row=row)


def bwd_bits(g, direct, res, self_graph):
    """What an order-independent kernel must store, as fp32 (gx, gsrc): the exact sums rounded once, the seed direct - g computed in
    fp32 and — self graph — added in fp32 (csrc/gkg_mr.hip: "o + (direct - gm)").  ``res``: mr_bwd's dict.  Compare with
    ``same_bits_z``: the sign of a ZERO gradient is not part of the contract (0 - g, -g and a -g seed that nothing is added to — the
    C oracle's — differ in it and in nothing else)."""
    g32 = np.asarray(g, dtype=np.float32)
    d32 = np.zeros_like(g32) if direct is None else np.asarray(direct, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sd = d32 - g32
        s32 = res["scat"].astype(np.float32)
        return (s32 + sd, None) if self_graph else (sd, s32)


def same_bits_z(got, want):
    """same_bits, with -0 and +0 taken as equal."""
    return same_bits(got + 0.0, want + 0.0)


def sum_bound(res, want):
    """|got - want| of ANY fp32 summation order of the destination's addends (self graph: the seed is one of them), first order:
    every one of the fan-in additions rounds a partial sum of magnitude <= sum |addend|, so the error is at most
    fan_in * 2^-24 * sum|addend|; 2 * 2^-24 * |want| covers the rounding of the seed and the second-order terms."""
    with np.errstate(invalid="ignore", over="ignore"):
        return res["fan"] * U24 * res["sabs"] + 2 * U24 * np.abs(want)


_NF_Q, _NF_R = (1, 2, 3, 4), (1, 2, 3, 3)       # 'nonfinite': queries carrying +inf, NaN, +inf, -inf and the rows they are sent to


def bwd_oor16(M):
    """u16 winning rows >= M (only M < 65536 has any)."""
    return ([M + 7] if M + 7 < 65535 else []) + [65535] if M < 65536 else []


def make_bwd_case(shape, kind, seed=0):
    """Inputs of one backward case -> dict: shape, kind, M, k, self; g, direct (BG, c, N) fp32; base (BG, N, k) int64 and slot_in
    (BG, c, N) u8 in range; idx / slot: the same with the int64 entries of oor_entries(M) and the slots 255 and k put where a
    gradient is routed through them; row16_in (BG, c, N) u16 in range, row16 with entries >= M (M < 65536); oor / oor_slot / oor16
    (the positions); dirty: (bg, ch) of the non-finite injections or None.  Half the lists name a few hot rows (rows 0 and M - 1
    among them) so that fan-ins are tens to hundreds; M == 65536 names rows 0 and 65535."""
    assert kind in BWD_KINDS + ("normal",)
    BG, c, N, M, k, self_graph = dims(shape)
    rng = np.random.default_rng([seed, 100 + (BWD_KINDS + ("normal",)).index(kind), BG, c, N, M, k])

    def draw(*s):
        if kind == "integer":
            return (rng.integers(-64, 65, size=s) / 8.0).astype(np.float32)
        if kind == "normal":
            return rng.standard_normal(size=s).astype(np.float32)
        mant = 1.0 + rng.integers(0, 2 ** 23, size=s) / 2.0 ** 23
        if kind == "tiny":
            return np.ldexp(mant, rng.integers(-130, -118, size=s)).astype(np.float32)
        return (np.ldexp(mant, rng.integers(-4, 4, size=s)) * rng.choice([-1.0, 1.0], size=s)).astype(np.float32)

    g, direct = draw(BG, c, N), draw(BG, c, N)
    hot = np.unique(np.concatenate([[0, M - 1], rng.integers(0, M, size=5)]))
    base = rng.integers(0, M, size=(BG, N, k), dtype=np.int64)
    base[:, ::2] = hot[rng.integers(0, len(hot), size=base[:, ::2].shape)]
    row16_in = rng.integers(0, M, size=(BG, c, N), dtype=np.int64)
    row16_in[:, :, 1::2] = hot[rng.integers(0, len(hot), size=row16_in[:, :, 1::2].shape)]
    slot_in = rng.integers(0, k, size=(BG, c, N)).astype(np.uint8)
    used = set()
    if M == 65536 and N > max(_Q_U16) and k >= 2:
        base[:, _Q_U16[0], :2] = (0, 65535)
        base[:, _Q_U16[1], :] = 65535
        base[:, _Q_U16[2], :] = 0
        row16_in[:, :, _Q_U16[0]] = 65535
        row16_in[:, :, _Q_U16[1]] = 0
        row16_in[:, 0, _Q_U16[2]] = 32768
        used |= set(_Q_U16)
    dirty = None
    if kind == "nonfinite" and N >= 8 and M >= 4:
        bg, ch = BG - 1, 1 % c
        dirty = (bg, ch)
        for q, r, v in zip(_NF_Q, _NF_R, (np.inf, np.nan, np.inf, -np.inf)):
            g[bg, ch, q] = v
            base[bg, q, 0], slot_in[bg, ch, q], row16_in[bg, ch, q] = r, 0, r
        used |= set(_NF_Q)
    idx, slot, row16, oor, oor_slot, oor16 = base.copy(), slot_in.copy(), row16_in.copy(), [], [], []
    free = [n for n in range(N) if n not in used] or list(range(N))
    pairs = [(b, n) for b in range(BG) for n in free]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    nonzero = lambda p: g.__setitem__(p, np.float32(0.125)) if g[p] == 0 else None      # noqa: E731
    for (b, n), e in zip(pairs[:5], oor_entries(M)):                    # channel 0 of the query goes through the entry
        idx[b, n, 0], slot[b, 0, n], slot_in[b, 0, n] = e, 0, 0
        nonzero((b, 0, n))
        oor.append((b, n, 0))
    for (b, n), e in zip(pairs[5:7], (255, k)):                         # channel c - 1 of the query names a slot >= k
        slot[b, c - 1, n] = e
        nonzero((b, c - 1, n))
        oor_slot.append((b, c - 1, n))
        p = ((b * N + n) * k + e) % idx.size                           # what a kernel without the slot clamp would read instead:
        if M > 1 and p != (b * N + n) * k + k - 1 and clamp(idx.reshape(-1)[p], M) == base[b, n, k - 1]:      # never the same row
            base[b, n, k - 1] = idx[b, n, k - 1] = (base[b, n, k - 1] + 1) % M
    for (b, n), e in zip(pairs[7:9] if len(pairs) >= 9 else pairs[:2], bwd_oor16(M)):
        row16[b, c - 1, n] = e
        nonzero((b, c - 1, n))
        oor16.append((b, c - 1, n))
    return dict(shape=shape, kind=kind, M=M, k=k, self=self_graph, g=g, direct=direct, base=base, slot_in=slot_in, idx=idx, slot=slot,
                row16_in=row16_in.astype(np.uint16), row16=row16.astype(np.uint16), oor=oor, oor_slot=oor_slot, oor16=oor16, dirty=dirty)


def bwd_expect(case, arg_kind, mode, in_range=False):
    """(res, (gx32, gsrc32)) of a case: mr_bwd's dict and bwd_bits' pair.  mode 0: direct = 0."""
    d = case["direct"] if mode == 1 else None
    if arg_kind == 1:
        res = mr_bwd(case["g"], case["row16_in" if in_range else "row16"], None, case["M"], case["self"], d)
    else:
        res = mr_bwd(case["g"], case["base" if in_range else "idx"], case["slot_in" if in_range else "slot"], case["M"], case["self"], d)
    return res, bwd_bits(case["g"], d, res, case["self"])


def exact_scale(kind):
    """2^s with g * 2^s an integer below 2^32 for every gradient of the kind: the grid its exact sums live on."""
    return {"integer": 3, "binades": 27, "nonfinite": 27, "tiny": 149}[kind]


# ---- the dispatch rule of gkg_mr_bwd_tm, restated (csrc/gkg_mr_plan.h mr_bwd_tm_plan; tests/test_mr_plan_host.py holds the two together) ----
def bwd_form(B, G, c, N, M, flags=0):
    """-> (form, chunk width or None).  Forms: 'stream' (fixed point, one sweep), 'stream-f64' (its fp64-atomic variant), 'two-sweep'
    (fixed point), 'private' / 'walk' (GKG_MR_DETERMINISTIC beyond the LDS budget), 'lds-f32' / 'global-f32' (fp32 atomics),
    'unsupported' (a forced streaming width that does not fit).  'stream' carries a detail: (threads, rows in flight, whole)."""
    C = G * c
    sv, fcw = (flags >> 16) & 3, (flags >> 8) & 0xFF
    div = lambda cw: C % cw == 0 and c % cw == 0                                           # noqa: E731
    fits8 = lambda cw, budget=LDS_BUDGET: M * cw * 8 + 16 <= budget and div(cw)            # noqa: E731
    one_launch = lambda cw: (C // cw) * (B + 7) < 0x7FFFFFFF                               # noqa: E731
    if N < 1 << 24 and (sv in (1, 2) or (sv == 0 and not flags & MR_F32 and N >= 160)):
        cw = fcw if (fcw and sv) else (16 if fits8(16) else 8 if fits8(8) else 4)
        if (sv and fits8(cw, 150 * 1024)) or fits8(cw):
            long_sweep = M > 512 and N >= 4 * M
            nt = 256 if (((flags >> 20) & 3) == 2 if sv else long_sweep) else 512
            u = 8 if (bool(flags & ROWS8) if sv else (M > 512 and not long_sweep)) else 4
            if sv == 2:
                nt, u = 512, 4
            return ("stream-f64" if sv == 2 else "stream"), cw, (nt, u, N <= (nt // (cw // 4)) * u)
        if sv:
            return "unsupported", None, None
    if not flags & MR_F32 and N < 1 << 24 and (M <= 512 or sv == 3 or flags & MR_DET):
        cw = fcw or (8 if fits8(8) else 4)
        if fits8(cw) and one_launch(cw):
            return "two-sweep", cw, None
    if flags & MR_DET:
        return ("private", 4, min(64, (144 * 1024) // (M * 16))) if (144 * 1024) // (M * 16) >= 1 else ("walk", 4, None)
    cw = 64
    while cw > 4 and (M * cw * 4 > LDS_BUDGET or not div(cw)):
        cw >>= 1
    while cw > 8 and (C // cw) * B < 512:
        cw >>= 1
    cw = fcw or cw
    return ("lds-f32", cw, None) if M * cw * 4 <= LDS_BUDGET and div(cw) and one_launch(cw) else ("global-f32", None, None)


FIXED_POINT = ("stream", "two-sweep")                        # order-independent AND exact on the kinds of BWD_KINDS
REPEATABLE = FIXED_POINT + ("stream-f64", "private", "walk")  # bits repeat from run to run (stream-f64: because its sums are exact here)


def bwd_stats_supported(B, G, c, N, M, mode, flags=0):
    """gkg_mr_bwd_tm_bnstats_supported, restated: mode 1, no measurement bits, and the rule picks a fixed-point form that is not a
    long-sweep (256-thread or 8-rows-in-flight) streaming instantiation."""
    if mode != 1 or (flags >> 16) & 3 or (flags >> 8) & 0xFF or flags & MR_F32:
        return False
    form, _, detail = bwd_form(B, G, c, N, M, flags)
    return form == "two-sweep" or (form == "stream" and detail[:2] == (512, 4))


# (shape (B, G, c, N, M | None, k), flags, form the rule must pick) — tests/test_hip_mr_bwd_abi.py runs every entry; the host test
# checks the third column against bwd_form and the exactness condition on every entry
TWO_SWEEP_SHAPES = [s for s in SHAPES_TM if (s[4] or s[3]) <= 512] + [(2, 1, 16, 159, None, 3), (1, 1, 8, 50, 512, 2)]
STREAM_SHAPES = [(2, 1, 16, 160, None, 3), (1, 2, 16, 513, 40, 2), (3, 2, 8, 200, None, 9), (9, 1, 12, 161, 37, 5), (9, 1, 16, 161, 37, 5),
                 (1, 1, 16, 600, 513, 2), (1, 1, 8, 2052, 513, 1), (1, 2, 8, 2052, 513, 1), (1, 1, 4, 160, 3071, 1), (1, 1, 16, 160, 3071, 1),
                 (2, 4, 4, 161, 37, 5)]
BWD_TM = ([(s, 0, "two-sweep") for s in TWO_SWEEP_SHAPES] + [(s, 0, "stream") for s in STREAM_SHAPES] + [
    ((1, 1, 8, 50, 513, 2), 0, "lds-f32"), ((1, 1, 4, 160, 3072, 1), 0, "lds-f32"),
    # forced forms (measurement bits): every chunk width that fits, <256 threads, 8 rows>, the fp64-atomic variant, the two-sweep kernel
    ((2, 1, 16, 160, None, 3), SV_STREAM | cw_bits(4), "stream"), ((2, 1, 16, 160, None, 3), SV_STREAM | cw_bits(8), "stream"),
    ((2, 1, 16, 160, None, 3), SV_STREAM | cw_bits(16) | NT256 | ROWS8, "stream"), ((2, 1, 16, 160, None, 3), SV_F64 | cw_bits(16), "stream-f64"),
    ((2, 1, 16, 160, None, 3), SV_TWO | cw_bits(16), "two-sweep"),
    ((1, 2, 16, 513, 40, 2), SV_STREAM | cw_bits(4) | NT256 | ROWS8, "stream"), ((1, 2, 16, 513, 40, 2), SV_STREAM | cw_bits(8), "stream"),
    ((1, 2, 16, 513, 40, 2), SV_F64 | cw_bits(8), "stream-f64"), ((1, 2, 16, 513, 40, 2), SV_TWO, "two-sweep"),
    ((2, 2, 40, 51, 300, 5), SV_STREAM | cw_bits(8), "stream"), ((2, 2, 40, 51, 300, 5), SV_F64 | cw_bits(4), "stream-f64"),
    ((1, 1, 16, 600, 513, 2), SV_STREAM | cw_bits(16) | NT256 | ROWS8, "stream"), ((1, 1, 16, 600, 513, 2), SV_F64 | cw_bits(16), "stream-f64"),
    # GKG_MR_DETERMINISTIC
    ((1, 1, 4, 50, 3071, 2), MR_DET, "two-sweep"), ((2, 1, 8, 50, 3072, 2), MR_DET, "private"), ((1, 2, 8, 50, 3072, 2), MR_DET, "private"),
    ((1, 1, 4, 70, 9216, 2), MR_DET, "private"), ((2, 2, 4, 20, 9217, 2), MR_DET, "walk"), ((1, 2, 8, 40, 65536, 4), MR_DET, "walk"),
    # GKG_MR_FP32_ATOMICS, and (above) the rule's own fp32 forms
    ((2, 2, 40, 51, 300, 5), MR_F32, "lds-f32"), ((1, 1, 4, 50, 6144, 2), MR_F32, "lds-f32"), ((1, 1, 16, 50, 6144, 2), MR_F32, "lds-f32"),
    ((1, 1, 4, 50, 6145, 2), MR_F32, "global-f32"), ((1, 2, 8, 40, 65536, 4), MR_F32, "global-f32"), ((1, 2, 8, 40, 65536, 4), 0, "global-f32"),
])


def bwd_id(entry):
    s, flags, form = entry
    return f"{shape_id(s)}-{form}-{flags:#x}"


def bwd_variants(shape):
    """A self-graph shape also runs as a bipartite graph over M = N keys (same form); a bipartite shape runs as it is."""
    return [shape, shape[:4] + (shape[3],) + shape[5:]] if shape[4] is None else [shape]
