"""Plain numpy/torch restatement of the max-relative aggregation's forward (include/gkg_hip.h: gkg_mr_fwd, gkg_mr_fwd_tm,
gkg_mr_fwd_tm16 and the operand producer of gkg_mr_linear_bf16), and the inputs the tests hold the kernels to it with.

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
