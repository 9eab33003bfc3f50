"""csrc/gkg_edge.hip through the C ABI against the fp64 reference of tests/edge_ref.py: the four gather entry points of EdgeConv
(conv='edge') and GraphSAGE (conv='sage', qc == NULL) of include/gkg_hip.h "EdgeConv aggregation".  a, c, mean0, invstd, mg, mgz and
argmax are test inputs, so the BN-statistics arithmetic of the Python wrapper stays out of the comparison.

Shapes (B, O, N, M, k) = edge_ref.SHAPES, each with qc given and qc = NULL:
    (1, 1, 1, 1, 1)          everything degenerate
    (2, 5, 255 / 256 / 257, 37, 9)   one thread short of a full workgroup, exactly one, a second one with a single live thread
    (3, 8, 513, 513, 3)      self graph: qs and qc are the same device buffer, as EdgeConv2d passes them
    (1, 20, 300, 5, 4)       five keys: almost every list repeats a key, 240 atomics per destination
    (2, 12, 64, 600, 255)    largest k (a uint8 argmax beyond 127)
    (4, 3, 70, 1000, 6)      M >> N, O no multiple of anything
Neighbour lists are randint (repeats), every third row repeats its first neighbour, two entries are out of range (-5, M + 7).

THE BAR (constants and report functions live in edge_ref so that tests/test_edge_reference_host.py, which shows on the CPU that
nine wrong formulas land above it, cannot drift from this file).  Error = |got - fp64| / scale, scale = |a z| + |c| of the edges
involved (forward) or the scatter of |a| (|g| act_grad_mag + |mg| + |zhat mgz|) (backward: |dz| term by term, edge_ref.bwd_mag).  Yardstick = the same formula in plain torch fp32
on the same operands.  The kernel must satisfy err <= max(4 * yardstick, 2^-22); the fp64-accumulated statistics, whose terms are
exact, 1e-12 of the sum of |term|.  Measured figures per shape: EXPERIMENTS.md "EdgeConv gather kernels vs fp64" (every test
prints its own with ``pytest -s``).  The argmax is never compared with an fp64 argmax for equality on random inputs: the fp64
value at the kernel's argmax must be within the bound of the fp64 maximum, for every element.  On integer-valued inputs every
fp32 operation is exact and everything, argmax included, is compared bit for bit.

Outputs sit between guard bands and are pre-filled; every test asserts the bands untouched."""
import pytest
import torch

import edge_ref as E
from util import Buf

pytestmark = pytest.mark.gpu

CASES = [(s, q) for s in E.SHAPES for q in (True, False)]
IDS = ["x".join(map(str, s)) + ("-qc" if q else "-null") for s, q in CASES]
K255 = (2, 12, 64, 600, 255)


# ------------------------------------------------------------------------------------------------------------------ helpers
def _L():
    from gkgnet_amd import _lib
    return _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    from gkgnet_amd.ops import _stream
    return _stream()


def _dev(k):
    """Device copies of a case's operands; a self graph keeps ONE buffer for qs and qc."""
    dv = {n: (v.cuda().contiguous() if torch.is_tensor(v) else v) for n, v in k.items()}
    if k.get("qc") is not None and k["qc"] is k["qs"]:
        dv["qc"] = dv["qs"]
    return dv


def _fwd(dv, code, want_arg=True):
    B, O, N, M, k = dv["shape"]
    out, arg = Buf((B, O, N)), (Buf((B, O, N), torch.uint8) if want_arg else None)
    _L().check(_L().load().gkg_edge_fwd(_p(dv["qs"]), _p(dv["qc"]), _p(dv["idx"]), _p(dv["a"]), _p(dv["c"]), _p(out.t),
                                        None if arg is None else _p(arg.t), B, O, N, M, k, code, _st()), "gkg_edge_fwd")
    torch.cuda.synchronize()
    assert out.guards_ok() and (arg is None or arg.guards_ok()), "gkg_edge_fwd wrote outside its outputs"
    return out.cpu(), (None if arg is None else arg.cpu())


def _bwd(dv, code, arg, dense, with_dqc=True):
    """-> (dqs, dqc or None) on the CPU.  ``arg``: uint8 (B, O, N) on the device."""
    B, O, N, M, k = dv["shape"]
    dqs, dqc = Buf((B, O, M), zero=True), (Buf((B, O, N)) if with_dqc else None)
    st = [dv[n] if dense else None for n in ("mean0", "invstd", "mg", "mgz")]
    _L().check(_L().load().gkg_edge_bwd(_p(dv["g"]), _p(dv["qs"]), _p(dv["qc"]), _p(dv["idx"]), _p(arg), _p(dv["a"]), _p(dv["c"]),
                                        _p(st[0]), _p(st[1]), _p(st[2]), _p(st[3]), _p(dqs.t), None if dqc is None else _p(dqc.t),
                                        B, O, N, M, k, code, _st()), "gkg_edge_bwd")
    torch.cuda.synchronize()
    assert dqs.guards_ok() and (dqc is None or dqc.guards_ok()), "gkg_edge_bwd wrote outside its outputs"
    return dqs.cpu(), (None if dqc is None else dqc.cpu())


def _sums(fn_name, dv, prefill, ptrs, code=None):
    """Call a statistics entry point on a (2 O) buffer pre-filled with ``prefill`` between guard bands; ``ptrs``: the arguments
    in front of ``sums``."""
    B, O, N, M, k = dv["shape"]
    s = Buf((2 * O,), torch.float64, fill=-7.0)
    s.t.fill_(prefill)
    tail = (B, O, N, M, k) if code is None else (B, O, N, M, k, code)
    _L().check(getattr(_L().load(), fn_name)(*ptrs, _p(s.t), *tail, _st()), fn_name)
    torch.cuda.synchronize()
    assert s.guards_ok(), fn_name + " wrote outside sums"
    return s.cpu()


def _z32(k):
    return E.z(k["qs"], k["qc"], k["idx"])


def _check_fwd(tag, out, arg, z32, a, c, code):
    rep = E.fwd_report(out, arg, z32, a, c, code)
    print(f"EDGE fwd  {tag} act {code}: yardstick {rep['yard']:.3e} out {rep['out']:.3e} pick {rep['pick']:.3e} "
          f"same {rep['same']:.3e} bound {rep['bound']:.3e}")
    assert rep["range"], (tag, code, "argmax outside [0, k)")
    assert bool(torch.isfinite(out).all()), (tag, code, "non-finite out")
    for name in ("out", "pick", "same"):
        assert rep[name] <= rep["bound"], (tag, code, name, rep)


def _check_bwd(tag, dqs, dqc, k, z32, arg, code, dense):
    st = {n: (k[n] if dense else None) for n in ("mean0", "invstd", "mg", "mgz")}
    rep = E.bwd_report(dqs, dqc, k["g"], z32, k["idx"], k["shape"][3], arg, k["a"], k["c"], code, **st)
    dqc_s = "-" if rep["dqc"] is None else f"{rep['dqc']:.3e}"
    print(f"EDGE bwd  {tag} act {code} {'dense' if dense else 'winner'}: dqs yardstick {rep['yard_dqs']:.3e} kernel {rep['dqs']:.3e} "
          f"bound {rep['bound_dqs']:.3e}; dqc yardstick {rep['yard_dqc']:.3e} kernel {dqc_s} bound {rep['bound_dqc']:.3e}")
    assert bool(torch.isfinite(dqs).all()) and (dqc is None or bool(torch.isfinite(dqc).all())), (tag, code, dense, "unwritten / non-finite")
    assert rep["dqs"] <= rep["bound_dqs"], (tag, code, dense, "dqs", rep)
    assert dqc is None or rep["dqc"] <= rep["bound_dqc"], (tag, code, dense, "dqc", rep)
    return rep


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("code", [0, 1, 2])
@pytest.mark.parametrize("shape,with_qc", CASES, ids=IDS)
def test_forward_against_fp64(shape, with_qc, code):
    k = E.make_case(shape, with_qc, E.case_seed(shape, with_qc))
    dv = _dev(k)
    out, arg = _fwd(dv, code)
    _check_fwd(f"{shape} qc={with_qc}", out, arg, _z32(k), k["a"], k["c"], code)
    out2, arg2 = _fwd(dv, code)
    assert torch.equal(out, out2) and torch.equal(arg, arg2), "two calls differ"
    out3, _ = _fwd(dv, code, want_arg=False)
    assert torch.equal(out, out3), "argmax == NULL changes out"


@pytest.mark.parametrize("code", [0, 1, 2])
def test_argmax_byte_beyond_127(code):
    """k = 255: rows whose unique maximum sits at position 254 and at position 128; the stored byte is that position."""
    shape = B, O, N, M, kk = K255
    k = E.make_case(shape, True, 77)
    gen = torch.Generator().manual_seed(78)
    k["idx"] = torch.randint(0, M - 2, (B, N, kk), generator=gen)                     # keys M-2 and M-1 appear nowhere else
    k["idx"][:, 0, 254], k["idx"][:, 1, 128] = M - 2, M - 1
    big = 100.0 * torch.sign(k["a"]).view(1, O)                                       # a z = +100 |a| in every channel
    k["qs"][:, :, M - 2], k["qs"][:, :, M - 1] = big, big
    out, arg = _fwd(_dev(k), code)
    assert bool((arg[:, :, 0] == 254).all()) and bool((arg[:, :, 1] == 128).all()), (arg[:, :, 0], arg[:, :, 1])
    _check_fwd(f"{shape} winners at 254 / 128", out, arg, _z32(k), k["a"], k["c"], code)
    _, _, arg64 = E.fwd(_z32(k).double(), k["a"].double(), k["c"].double(), code)
    assert torch.equal(arg[:, :, :2].long(), arg64[:, :, :2])


# ------------------------------------------------------------------------------------------------------------------ exact arithmetic
@pytest.mark.parametrize("shape,with_qc", CASES, ids=IDS)
def test_exact_arithmetic_bit_for_bit(shape, with_qc):
    """Integer-valued operands: every fp32 product, difference and fma of the kernels is exact, every sum independent of its
    order.  out, argmax (first maximum among many exact ties), the statistics and the winner-only backward equal fp64 exactly.
    An off-by-one in the gather, the clamp, the tie rule or the scatter target shows here."""
    B, O, N, M, kk = shape
    k = E.make_exact_case(shape, with_qc, E.case_seed(shape, with_qc))
    dv = _dev(k)
    z64 = _z32(k).double()
    assert torch.equal(z64, E.z(k["qs"].double(), None if k["qc"] is None else k["qc"].double(), k["idx"]))   # the difference is exact
    ref_s, _ = E.stats(z64)
    got_s = _sums("gkg_edge_stats", dv, 0.0, [_p(dv[n]) for n in ("qs", "qc", "idx")])
    assert torch.equal(got_s, ref_s), ("stats", shape, with_qc, (got_s - ref_s).abs().max())
    for code in (0, 2):
        out64, _, arg64 = E.fwd(z64, k["a"].double(), k["c"].double(), code)
        out, arg = _fwd(dv, code)
        assert torch.equal(out.double(), out64), ("out", shape, with_qc, code, int((out.double() != out64).sum()))
        assert torch.equal(arg.long(), arg64), ("argmax", shape, with_qc, code, int((arg.long() != arg64).sum()))
        r_s, r_c = E.bwd(k["g"].double(), z64, k["idx"], M, arg64, k["a"].double(), k["c"].double(), code)
        arg_d = arg.cuda()
        for turn in range(2):
            dqs, dqc = _bwd(dv, code, arg_d, dense=False)
            assert torch.equal(dqs.double(), r_s), ("dqs", shape, with_qc, code, turn, int((dqs.double() != r_s).sum()))
            assert torch.equal(dqc.double(), r_c), ("dqc", shape, with_qc, code, turn, int((dqc.double() != r_c).sum()))


# ------------------------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("shape,with_qc", CASES, ids=IDS)
def test_statistics_against_fp64(shape, with_qc):
    """gkg_edge_stats and gkg_edge_bwd_stats accumulate fp32-rounded terms in fp64 and ADD into ``sums``.  Where the terms are
    reproducible exactly (z; g' and zhat for act 0 and 2: g' is g or 0, zhat two IEEE fp32 operations) only the order of the fp64
    additions differs: 1e-12 of the sum of |term|.  With GELU g' carries fp32 roundings of its own: the fp32 bar applies."""
    B, O, N, M, kk = shape
    k = E.make_case(shape, with_qc, E.case_seed(shape, with_qc))
    dv = _dev(k)
    z32 = _z32(k)
    z64 = z32.double()
    tag = f"{shape} qc={with_qc}"
    pre = 1000.5
    ref, mag = E.stats(z64)
    got = _sums("gkg_edge_stats", dv, pre, [_p(dv[n]) for n in ("qs", "qc", "idx")])
    err = E.rel(got, ref + pre, mag + pre)
    print(f"EDGE sums {tag} stats: err {err:.3e} (bound {E.SUM_TOL:.0e})")
    assert err <= E.SUM_TOL, (tag, "gkg_edge_stats", err)
    a64, c64, m64, i64, g64 = (k[n].double() for n in ("a", "c", "mean0", "invstd", "g"))
    for code in (0, 1, 2):
        _, arg = _fwd(dv, code)
        arg_d = arg.cuda()
        got = _sums("gkg_edge_bwd_stats", dv, pre, [_p(dv["g"]), _p(dv["qs"]), _p(dv["qc"]), _p(dv["idx"]), _p(arg_d), _p(dv["a"]),
                                                    _p(dv["c"]), _p(dv["mean0"]), _p(dv["invstd"])], code)
        ref, mag = E.bwd_stats(g64, z64, arg, a64, c64, m64, i64, code)
        yard, _ = E.bwd_stats(k["g"], z32, arg, k["a"], k["c"], k["mean0"], k["invstd"], code)
        y = E.rel(yard, ref, mag)
        if code == 1:
            err, bnd = E.rel(got - pre, ref, mag), E.bound(y)
        else:
            gp64, _, gm64 = E.bwd_terms(g64, z64, arg, a64, c64, m64, i64, code)
            _, zhat32, _ = E.bwd_terms(k["g"], z32, arg, k["a"], k["c"], k["mean0"], k["invstd"], code)
            ref, mag = E.term_sums(gp64, zhat32.double(), gm64)
            err, bnd = E.rel(got, ref + pre, mag + pre), E.SUM_TOL
        print(f"EDGE sums {tag} bwd_stats act {code}: err {err:.3e} bound {bnd:.3e} (fp32 yardstick vs fp64 {y:.3e})")
        assert err <= bnd, (tag, "gkg_edge_bwd_stats", code, err, bnd)


# ------------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("dense", [True, False], ids=["dense", "winner"])
@pytest.mark.parametrize("code", [0, 1, 2])
@pytest.mark.parametrize("shape,with_qc", CASES, ids=IDS)
def test_backward_against_fp64(shape, with_qc, code, dense):
    """The argmax is the kernel's own forward's.  dqc is passed in both forms; with qc == NULL it may be omitted, and dqs must then
    hold the same values (to the bound: fp32 atomics arrive in any order)."""
    k = E.make_case(shape, with_qc, E.case_seed(shape, with_qc))
    dv = _dev(k)
    z32 = _z32(k)
    tag = f"{shape} qc={with_qc}"
    _, arg = _fwd(dv, code)
    arg_d = arg.cuda()
    dqs, dqc = _bwd(dv, code, arg_d, dense)
    _check_bwd(tag, dqs, dqc, k, z32, arg, code, dense)
    if not with_qc:
        dqs2, none = _bwd(dv, code, arg_d, dense, with_dqc=False)
        assert none is None
        _check_bwd(tag + " dqc=NULL", dqs2, None, k, z32, arg, code, dense)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "winner"])
@pytest.mark.parametrize("with_qc", [True, False])
def test_backward_with_a_synthetic_argmax(with_qc, dense):
    """argmax = randint(0, k): the backward is held to the reference on an argmax no forward produced (decouples the two kernels)."""
    shape = (2, 5, 257, 37, 9)
    k = E.make_case(shape, with_qc, E.case_seed(shape, with_qc))
    dv = _dev(k)
    dqs, dqc = _bwd(dv, 1, dv["arg_rand"], dense)
    _check_bwd(f"{shape} qc={with_qc} synthetic argmax", dqs, dqc, k, _z32(k), k["arg_rand"], 1, dense)


# ------------------------------------------------------------------------------------------------------------------ non-finite
@pytest.mark.parametrize("code", [0, 1, 2])
@pytest.mark.parametrize("with_qc", [True, False])
def test_nan_and_inf_reach_exactly_the_rows_that_gather_them(with_qc, code):
    """One NaN and one +inf in single Q elements.  Exactly the outputs (b0, o0, n) whose clamped list holds j0 are NaN (+inf where
    the inf element is gathered, in a channel with a > 0); every other output is finite and bit-identical to the clean run."""
    shape = B, O, N, M, kk = (2, 5, 257, 37, 9)
    k = E.make_case(shape, with_qc, E.case_seed(shape, with_qc))
    clean, _ = _fwd(_dev(k), code)
    (b0, o0, j0), (b1, o1, j1) = (0, 1, 11), (1, 0, 36)                    # a[1] < 0, a[0] > 0; key 36 = M - 1 also takes the clamped M + 7
    assert float(k["a"][o0]) < 0 < float(k["a"][o1])
    k["qs"] = k["qs"].clone()
    k["qs"][b0, o0, j0], k["qs"][b1, o1, j1] = float("nan"), float("inf")
    out, arg = _fwd(_dev(k), code)
    j = E.clamp(k["idx"], M)
    want_nan = torch.zeros(B, O, N, dtype=torch.bool)
    want_inf = torch.zeros(B, O, N, dtype=torch.bool)
    want_nan[b0, o0] = (j[b0] == j0).any(-1)
    want_inf[b1, o1] = (j[b1] == j1).any(-1)
    assert int(want_nan.sum()) > 0 and int(want_inf.sum()) > 0 and bool((j[-1, -1] == j1).any())
    assert torch.equal(torch.isnan(out), want_nan), (int(torch.isnan(out).sum()), int(want_nan.sum()))
    assert torch.equal(out == float("inf"), want_inf), (int((out == float("inf")).sum()), int(want_inf.sum()))
    rest = ~(want_nan | want_inf)
    assert bool(torch.isfinite(out[rest]).all()) and torch.equal(out[rest], clean[rest])
    assert bool((arg < kk).all())
    hit = j.unsqueeze(1).expand(B, O, N, kk).gather(-1, arg.long().unsqueeze(-1)).squeeze(-1)     # the key each argmax points at
    assert bool((hit[want_nan] == j0).all()) and bool((hit[want_inf] == j1).all())


# ------------------------------------------------------------------------------------------------------------------ rejections
def test_bad_arguments_are_rejected_before_any_launch():
    from gkgnet_amd import _abi
    lib, err_shape = _L().load(), _abi.header().constants["ERR_SHAPE"]
    shape = B, O, N, M, kk = (2, 3, 10, 7, 4)
    k = E.make_case(shape, True, 5)
    dv = _dev(k)
    out, arg, dqs, dqc = Buf((B, O, N)), Buf((B, O, N), torch.uint8), Buf((B, O, M), zero=True), Buf((B, O, N))
    sums = Buf((2 * O,), torch.float64, fill=-7.0)
    argin = dv["arg_rand"]
    before = [t.full.clone() for t in (out, arg, dqs, dqc, sums)]
    st = _st()
    base = dict(g=_p(dv["g"]), qs=_p(dv["qs"]), qc=_p(dv["qc"]), idx=_p(dv["idx"]), argin=_p(argin), a=_p(dv["a"]), c=_p(dv["c"]),
                mean0=_p(dv["mean0"]), invstd=_p(dv["invstd"]), mg=_p(dv["mg"]), mgz=_p(dv["mgz"]), out=_p(out.t), arg=_p(arg.t),
                dqs=_p(dqs.t), dqc=_p(dqc.t), sums=_p(sums.t), B=B, O=O, N=N, M=M, k=kk, act=1)
    order = {"gkg_edge_stats": "qs qc idx sums B O N M k",
             "gkg_edge_fwd": "qs qc idx a c out arg B O N M k act",
             "gkg_edge_bwd_stats": "g qs qc idx argin a c mean0 invstd sums B O N M k act",
             "gkg_edge_bwd": "g qs qc idx argin a c mean0 invstd mg mgz dqs dqc B O N M k act"}

    def call(fn, **kw):
        v = dict(base)
        v.update(kw)
        return getattr(lib, fn)(*[v[n] for n in order[fn].split()], st)

    def rejected(fn, code=None, **kw):
        rc = call(fn, **kw)
        assert rc != 0, (fn, kw, "accepted")
        assert len(lib.gkg_last_error_string()) > 0, (fn, kw, "no error string")
        if code is not None:
            assert rc == code, (fn, kw, rc)

    for fn in order:
        rejected(fn, qs=None)
        rejected(fn, idx=None)
        for dim in "BONMk":
            rejected(fn, **{dim: 0})
            rejected(fn, **{dim: -3})
        rejected(fn, k=256)
        rejected(fn, O=65536)
        rejected(fn, B=65536)
        if "act" in order[fn]:
            rejected(fn, err_shape, act=3)                                   # a value error, not a null pointer
            rejected(fn, act=-1)
    for name in ("out", "a", "c"):
        rejected("gkg_edge_fwd", **{name: None})
    rejected("gkg_edge_stats", sums=None)
    for name in ("g", "argin", "a", "c", "mean0", "invstd", "sums"):
        rejected("gkg_edge_bwd_stats", **{name: None})
    for name in ("g", "argin", "a", "c", "dqs"):
        rejected("gkg_edge_bwd", **{name: None})
    rejected("gkg_edge_bwd", dqc=None)                                      # qc without dqc
    for name in ("mgz", "mean0", "invstd"):
        rejected("gkg_edge_bwd", **{name: None})                            # mg without the rest of the batch-statistics set
    torch.cuda.synchronize()
    for t, b in zip((out, arg, dqs, dqc, sums), before):
        same = (t.full == b) | ((t.full != t.full) & (b != b)) if t.full.is_floating_point() else (t.full == b)
        assert bool(same.all()), "a rejected call wrote to an output"
    # the same arguments, unmodified, are accepted (the rejections above are about the one argument each one changes)
    for fn in order:
        assert call(fn) == 0, fn
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ bounded random pass
def test_thirty_random_problems():
    import random
    rng = random.Random(20240607)
    for i in range(30):
        shape = (rng.randint(1, 4), rng.randint(1, 24), rng.choice([1, 7, 63, 64, 65, 255, 256, 257, 300]), rng.randint(1, 400),
                 rng.randint(1, 40))
        code, with_qc, dense = rng.randint(0, 2), rng.random() < 0.5, rng.random() < 0.5
        tag = f"random #{i} {shape} qc={with_qc}"
        k = E.make_case(shape, with_qc, 5000 + i)
        dv = _dev(k)
        z32 = _z32(k)
        out, arg = _fwd(dv, code)
        _check_fwd(tag, out, arg, z32, k["a"], k["c"], code)
        dqs, dqc = _bwd(dv, code, arg.cuda(), dense, with_dqc=with_qc or rng.random() < 0.5)
        _check_bwd(tag, dqs, dqc, k, z32, arg, code, dense)
