"""The host-side protocol of the k-NN's prepared tokens (gkgnet_amd/knn_prep.py) on the CPU: the real KnnProblem and
consumer_ws_flags with CPU tensors and a stub library whose only entry point is the size query, which counts its calls."""
import ctypes as C

import pytest
import torch

from gkgnet_amd import _abi, _lib, knn_prep
from gkgnet_amd.knn_prep import KnnProblem

WS_BYTES = 4096
FIELDS = ("B", "G", "c", "N", "M", "k", "d", "has_y", "has_rp", "flags", "fused_mr")
CPU = torch.device("cpu")


class _Lib:
    def __init__(self):
        self.queries = []

    def gkg_knn_workspace_bytes(self, *args):
        self.queries.append(args)
        return WS_BYTES


def _base():
    """A label graph's problem as a consumer spells it: B, G, c, N, M, k, d, has_y, has_rp, flags, fused_mr."""
    return dict(B=3, G=2, c=32, N=20, M=144, k=9, d=1, has_y=1, has_rp=0, flags=knn_prep.problem_flags(None), fused_mr=1)


def _problem(f):
    return KnnProblem(f["B"], f["G"], f["c"], f["N"], f["M"], f["k"], f["d"], f["has_y"], torch.zeros(1) if f["has_rp"] else None,
                      f["fused_mr"], f["flags"])


def _consume(lib, x, f):
    return knn_prep.consumer_ws_flags(lib, x, *(f[n] for n in FIELDS))


# ------------------------------------------------------------------------------------------------ one spelling
@pytest.mark.parametrize("select,prefilter", [("", ""), ("buffered", ""), ("direct", ""), ("", "0"), ("", "force"), ("direct", "force")])
def test_problem_flags_is_the_expression_it_replaces(monkeypatch, select, prefilter):
    monkeypatch.setenv("GKG_KNN_SELECT", select)
    monkeypatch.setenv("GKG_KNN_PREFILTER", prefilter)
    rp = torch.zeros(1, 4, 4)
    for unit in (0, _lib.KNN_RELPOS_UNIT):
        monkeypatch.setattr(_lib, "relpos_flags", lambda t, unit=unit: 0 if t is None else unit)
        for t in (None, rp):
            want = _lib.KNN_NORMALIZE | _lib.knn_select_flags() | _lib.relpos_flags(t)
            assert knn_prep.problem_flags(t) == want
            assert knn_prep.problem_flags(t, True) == want | _lib.KNN_BF16_CONTRACT
            assert KnnProblem(1, 1, 4, 8, 8, 2, 1, False, t, False).flags == want


# ------------------------------------------------------------------------------------------------ queries
def test_marked_queries_yield_the_producers_workspace():
    lib, f = _Lib(), _base()
    p = _problem(f)
    x = torch.zeros(4)
    p.producer_args(lib, x, None, None, 8, 2)              # the producer ran: the workspace exists
    p.mark(x)
    ws, flags = _consume(lib, x, f)
    assert ws is p.ws and flags == f["flags"] | _lib.KNN_X_PREPARED
    assert len(lib.queries) == 1                                # ... and the consumer asked for no other


@pytest.mark.parametrize("field", FIELDS)
def test_any_differing_field_yields_a_fresh_workspace(field):
    lib, f = _Lib(), _base()
    p = _problem(f)
    x = torch.zeros(4)
    p.workspace(lib, CPU)
    p.mark(x)
    g = dict(f)
    g[field] = (1 - f[field]) if field in ("has_y", "has_rp", "fused_mr") else \
        (f[field] ^ _lib.KNN_NO_PREFILTER) if field == "flags" else f[field] + 1
    ws, flags = _consume(lib, x, g)
    assert ws is not p.ws and ws.numel() == WS_BYTES and flags == g["flags"]
    assert lib.queries[-1] == (g["B"] * g["G"], g["c"], g["N"], g["M"], g["k"], g["d"], _lib.F32, _lib.KNN_NORMALIZE)


def test_unmarked_or_unprepared_queries_yield_a_fresh_workspace():
    lib, f = _Lib(), _base()
    ws, flags = _consume(lib, torch.zeros(4), f)
    assert ws.numel() == WS_BYTES and flags == f["flags"]
    x = torch.zeros(4)
    _problem(f).mark(x)                                         # marked, but no producer ever allocated a workspace
    ws, flags = _consume(lib, x, f)
    assert ws.numel() == WS_BYTES and flags == f["flags"] and len(lib.queries) == 2


def test_bf16_contract_never_reads_prepared_queries():
    lib, f = _Lib(), _base()
    f["flags"] |= _lib.KNN_BF16_CONTRACT
    p = _problem(f)                                             # even a producer that (wrongly) claimed the same flag word
    x = torch.zeros(4)
    p.workspace(lib, CPU)
    p.mark(x)
    ws, flags = _consume(lib, x, f)
    assert ws is not p.ws and flags == f["flags"]


# ------------------------------------------------------------------------------------------------ keys
def _label_knn(f):
    return (f["G"], f["N"], f["k"], f["d"], f["fused_mr"])


def test_adopted_keys_share_the_workspace_and_set_y_prepared():
    lib, f = _Lib(), _base()
    keys = KnnProblem.keys_for_label(f["B"], f["G"] * f["c"], f["M"], _label_knn(f))
    assert keys.as_keys == 1 and keys.tuple() == _problem(f).tuple() and keys.ws is None
    out_tm = torch.zeros(4)
    keys.producer_args(lib, torch.zeros(4), out_tm, torch.zeros(4), 8, 2)
    keys.mark(out_tm)
    assert knn_prep.prepared_keys(out_tm) is keys
    p = _problem(f)
    assert p.adopt_keys(knn_prep.prepared_keys(out_tm)) is True
    assert p.ws is keys.ws and p.y_ready
    x = torch.zeros(4)
    p.mark(x)                                                   # fc1 adds the queries to the same workspace
    ws, flags = _consume(lib, x, f)
    assert ws is keys.ws and flags == f["flags"] | _lib.KNN_X_PREPARED | _lib.KNN_Y_PREPARED
    assert len(lib.queries) == 1
    ws, flags = _consume(lib, out_tm, f)                        # the keys' mark does not make out_tm anybody's prepared queries
    assert ws is not keys.ws and flags == f["flags"]


def test_adopt_keys_refuses_anything_else():
    lib, f = _Lib(), _base()
    p = _problem(f)
    assert p.adopt_keys(None) is False
    keys = KnnProblem.keys_for_label(f["B"], f["G"] * f["c"], f["M"], _label_knn(f))
    assert p.adopt_keys(keys) is False                          # equal tuple, but the producer never ran (no workspace)
    other = KnnProblem.keys_for_label(f["B"], f["G"] * f["c"], f["M"] + 1, _label_knn(f))
    other.workspace(lib, CPU)
    assert p.adopt_keys(other) is False                         # another problem's keys
    assert p.ws is None and not p.y_ready
    assert knn_prep.prepared_keys(torch.zeros(1)) is None


def test_keys_for_label_refuses_widths_the_kernel_does_not_take():
    assert KnnProblem.keys_for_label(2, 64, 144, None) is None
    assert KnnProblem.keys_for_label(2, 64, 144, (3, 20, 9, 1, True)) is None       # C % G2
    assert KnnProblem.keys_for_label(2, 36, 144, (6, 20, 9, 1, True)) is None       # (C // G2) % 4
    keys = KnnProblem.keys_for_label(2, 64, 144, (2, 20, 9, 1, True))
    assert keys.tuple() == (2, 2, 32, 20, 144, 9, 1, 1, 0, knn_prep.problem_flags(None), 1)


# ------------------------------------------------------------------------------------------------ announcement
def test_announce_stores_the_label_graph_only_when_it_changed():
    mod = torch.nn.Identity()
    assert knn_prep.announced(mod) is None
    p = _problem(_base())
    p.announce(None, 2, 20)                                     # no known producer: nothing to tell
    p.announce(mod, 2, 20)
    first = knn_prep.announced(mod)
    assert first == (2, 20, 9, 1, 1)
    _problem(_base()).announce(mod, 2, 20)                      # the same graph again, a new problem object
    assert knn_prep.announced(mod) is first
    g = _base()
    g["k"] = 7
    _problem(g).announce(mod, 2, 20)
    assert knn_prep.announced(mod) == (2, 20, 7, 1, 1)
    assert KnnProblem.keys_for_label(3, 64, 144, knn_prep.announced(mod)).tuple() == _problem(dict(g, M=144)).tuple()


# ------------------------------------------------------------------------------------------------ laziness
def test_the_workspace_is_sized_on_first_use_and_once():
    lib, f = _Lib(), _base()
    p = _problem(f)
    keys = KnnProblem.keys_for_label(f["B"], f["G"] * f["c"], f["M"], _label_knn(f))
    assert lib.queries == [] and p.ws is None and keys.ws is None
    ws = p.workspace(lib, CPU)
    assert p.workspace(lib, CPU) is ws and p.producer_args(lib, torch.zeros(4), None, None, 8, 2)[-2] == ws.data_ptr()
    assert lib.queries == [(f["B"] * f["G"], f["c"], f["N"], f["M"], f["k"], f["d"], _lib.F32, _lib.KNN_NORMALIZE)]
    assert ws.dtype == torch.uint8 and ws.numel() == WS_BYTES


# ------------------------------------------------------------------------------------------------ the producers' argument run
def _matches_prototype(run):
    """``run`` against gkg_affine_knn_prep's parameters 3..-1 (out .. knn_workspace_bytes) as the header declares them."""
    argtypes = _abi.header().protos["gkg_affine_knn_prep"][1][3:-1]
    assert len(run) == len(argtypes)
    for v, t in zip(run, argtypes):
        if t is C.c_void_p:
            assert v is None or type(v) is int
        else:
            assert t in (C.c_int, C.c_uint, C.c_size_t) and type(v) is int and v >= 0
    for name in ("gkg_bn_apply_knn_prep", "gkg_bn_apply_knn_prep_sync"):     # the same run behind the BN pass's own head
        assert _abi.header().protos[name][1][12:12 + len(argtypes)] == argtypes


def test_producer_args_of_a_queries_problem():
    lib, f = _Lib(), _base()
    kp = _problem(f)
    out, out_tm, res = torch.zeros(8), None, None
    ldo, ochunk = 128, 16
    run = kp.producer_args(lib, out, out_tm, res, ldo, ochunk)
    assert run == (out.data_ptr(), ldo, ochunk, kp.B, kp.G, kp.c, kp.N, kp.M, kp.k, kp.d, kp.has_y, kp.has_rp, kp.flags, kp.fused_mr,
                   0, None, None, kp.ws.data_ptr(), kp.ws.numel())
    _matches_prototype(run)


def test_producer_args_of_a_keys_problem():
    lib, f = _Lib(), _base()
    kp = KnnProblem.keys_for_label(f["B"], f["G"] * f["c"], f["M"], _label_knn(f))
    out, out_tm, res = torch.zeros(8), torch.zeros(8), torch.zeros(8)
    run = kp.producer_args(lib, out, out_tm, res, 64, 0)
    assert run == (out_tm.data_ptr(), 0, 0, kp.B, kp.G, kp.c, kp.N, kp.M, kp.k, kp.d, kp.has_y, kp.has_rp, kp.flags, kp.fused_mr,
                   1, res.data_ptr(), out.data_ptr(), kp.ws.data_ptr(), kp.ws.numel())
    _matches_prototype(run)
    assert len({out.data_ptr(), out_tm.data_ptr(), res.data_ptr(), kp.ws.data_ptr()}) == 4      # a transposition would show
