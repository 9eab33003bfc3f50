"""gkg_linear_bf16_knn_prep (csrc/gkg_linear_bf16.hip): a Grapher's fc1 under bf16 autocast and the token preparation of the k-NN
call behind it as ONE launch (reference torch_vertex.py:326 -> torch_edge.py:167-173).  Bit for bit throughout: `out` against
gkg_linear_bf16, the whole k-NN workspace against gkg_affine_knn_prep fed the raw accumulators, the graphs of the prepared call
against the unprepared call and the C oracle — then the dispatch from ``fused`` under GKG_ENABLE=lin_bf16,lin_bf16_prep."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
S32 = 0x7FC12345          # a NaN pattern no kernel writes

# (B, G, c, N, M (None: self graph), cin, k, d, relative_pos, extra flags)
PF = "pf"                 # GKG_KNN_FORCE_PREFILTER | GKG_KNN_RELPOS_UNIT
CASES = {
    "1-straddle": (2, 2, 40, 324, None, 80, 9, 1, True, None),     # 648 rows: partial last row tile, a tile across the image boundary
    "2": (1, 4, 80, 200, None, 320, 9, 2, False, None),
    "3-wide": (2, 2, 320, 81, None, 640, 9, 3, True, None),        # widest group: one group spans several column tiles
    "4-128col": (8, 2, 320, 829, None, 160, 9, 1, False, None),    # 52 row tiles x 5 column tiles >= 256: the 128-column form
    "5-narrow": (2, 8, 12, 196, None, 96, 18, 2, False, None),     # pvig_m's groups, k d = 36, the 12-padding of cpad
    "6-pooled": (1, 2, 40, 1296, 324, 80, 9, 1, True, None),       # keys given: only the queries are prepared
    "7-small": (1, 2, 40, 81, None, 80, 9, 1, False, None),        # fewer rows than one tile
    "8-pf-1": (2, 2, 40, 324, None, 80, 9, 1, True, PF),
    "8-pf-3": (2, 2, 320, 81, None, 640, 9, 3, True, PF),          # un-split: hi / lo planes, pad rows 81..95
    "8-pf-200": (1, 2, 200, 330, None, 400, 9, 2, False, PF),
    # two more shapes whose plan is known to keep the keys un-split (M <= 256, or >= 256 query tiles), so that the planes exist:
    # images across row tiles with pad rows 200..223, and many small groups
    "8-pf-tiles": (3, 2, 40, 200, None, 80, 9, 1, True, PF),
    "8-pf-many": (16, 4, 20, 330, None, 80, 9, 1, False, PF),
    # one column tile holds every group (no hand-off between workgroups): 64 columns, and 128 columns at >= 256 row tiles
    "9-one-tile-64": (3, 2, 32, 200, None, 64, 9, 1, True, None),
    "9-one-tile-64-pf": (3, 2, 32, 200, None, 64, 9, 1, True, PF),
    "9-one-tile-128": (16, 2, 40, 2100, 100, 80, 9, 1, False, None),
}


def _planes(w16):
    from gkgnet_amd import _lib
    co, ci = w16.shape
    ci_pad, co_pad = (ci + 15) // 16 * 16, (co + 31) // 32 * 32
    W = torch.zeros((co_pad, ci_pad), dtype=BF16, device=w16.device)
    W[:co, :ci] = w16
    p = W.view(co_pad, ci_pad // 8, 8).permute(1, 0, 2).contiguous()
    assert p.numel() * 2 == _lib.load().gkg_linear_bf16_planes_bytes(ci, co)
    return p


@functools.lru_cache(maxsize=None)
def _problem(name):
    """The operands of a case, fixed per case and never modified."""
    from gkgnet_amd import _lib
    B, G, c, N, M, cin, k, d, relpos, extra = CASES[name]
    C, Mk = G * c, (N if M is None else M)
    g = torch.Generator(device="cuda").manual_seed(1000 * cin + 7 * N + c)
    x = torch.randn(B * N, cin, device="cuda", generator=g).to(BF16)
    w = (torch.randn(C, cin, device="cuda", generator=g) / cin ** 0.5).to(BF16)
    a = torch.rand(C, device="cuda", generator=g) + 0.5
    sign = torch.where(torch.rand(C, device="cuda", generator=g) < 0.5, -1.0, 1.0)
    cs = sign * (torch.rand(C, device="cuda", generator=g) * 0.3 + 0.2)          # away from 0: a zero accumulator's sign cannot matter
    y = None if M is None else torch.randn(B, Mk, C, device="cuda", generator=g)
    rp = (-torch.rand(N, Mk, device="cuda", generator=g)) if relpos else None
    flags = _lib.KNN_NORMALIZE | (_lib.KNN_FORCE_PREFILTER | _lib.KNN_RELPOS_UNIT if extra == PF else 0)
    return dict(B=B, G=G, c=c, N=N, M=Mk, cin=cin, k=k, d=d, C=C, R=B * N, x=x, planes=_planes(w), a=a, cs=cs, y=y, rp=rp, flags=flags)


def _linear(p, a, cs, out=None, ldo=None):
    from gkgnet_amd import _lib
    o = torch.empty(p["R"], p["C"], device="cuda") if out is None else out
    _lib.check(_lib.load().gkg_linear_bf16(p["x"].data_ptr(), p["cin"], p["planes"].data_ptr(), None if a is None else a.data_ptr(),
                                           cs.data_ptr(), None, 0, o.data_ptr(), ldo or p["C"], None, 0, p["R"], p["cin"], p["C"], 0,
                                           None), "gkg_linear_bf16")
    return o


def _wsb(p):
    from gkgnet_amd import _lib
    return int(_lib.load().gkg_knn_workspace_bytes(p["B"] * p["G"], p["c"], p["N"], p["M"], p["k"], p["d"], _lib.F32, _lib.KNN_NORMALIZE))


def _run_args(p, out, ldo, ws, ochunk=0, as_keys=0):
    """The producers' shared argument run, `out` .. `knn_workspace_bytes`."""
    return (out.data_ptr(), ldo, ochunk, p["B"], p["G"], p["c"], p["N"], p["M"], p["k"], p["d"], 0 if p["y"] is None else 1,
            0 if p["rp"] is None else 1, p["flags"], 0, as_keys, None, None, ws.data_ptr(), ws.numel())


def _scratch(p):
    from gkgnet_amd import _lib
    n = int(_lib.load().gkg_linear_bf16_knn_prep_scratch_bytes(p["R"]))
    assert n == 4 * ((p["R"] + 127) // 128)
    return torch.zeros(n // 4, dtype=torch.int32, device="cuda")


def _fused(p, out, ldo, ws, scratch, x=None, cin=None, **kw):
    from gkgnet_amd import _lib
    x = p["x"] if x is None else x
    return _lib.load().gkg_linear_bf16_knn_prep(x.data_ptr(), x.stride(0), p["planes"].data_ptr(), p["cin"] if cin is None else cin,
                                                p["a"].data_ptr(), p["cs"].data_ptr(), *_run_args(p, out, ldo, ws, **kw),
                                                scratch.data_ptr(), scratch.numel() * 4, None)


def _graph(p, x_tm, ws, prepared):
    from gkgnet_amd import _lib
    nn16 = torch.empty((p["B"] * p["G"], p["N"], p["k"]), dtype=torch.int16, device="cuda")
    f = p["flags"] | (_lib.KNN_X_PREPARED if prepared else 0)
    _lib.check(_lib.load().gkg_knn_fwd_tm16(x_tm.data_ptr(), 0, 0, None if p["y"] is None else p["y"].data_ptr(),
                                            None if p["rp"] is None else p["rp"].data_ptr(), nn16.data_ptr(), p["B"], p["G"], p["c"],
                                            p["N"], p["M"], p["k"], p["d"], _lib.F32, f, ws.data_ptr(), ws.numel(), None),
               "gkg_knn_fwd_tm16")
    return nn16


@pytest.mark.parametrize("name", list(CASES))
def test_one_launch_gives_the_bits_of_projection_plus_preparation(name):
    from gkgnet_amd import _lib
    from oracle import c_oracle as O
    lib = _lib.load()
    p = _problem(name)
    B, G, c, N, C, R = p["B"], p["G"], p["c"], p["N"], p["C"], p["R"]
    assert lib.gkg_linear_bf16_knn_prep_supported(p["cin"], B, G, c, N, p["M"], p["k"], p["d"], 0 if p["y"] is None else 1,
                                                  0 if p["rp"] is None else 1, p["flags"], 0) == 1
    acc = _linear(p, None, torch.zeros(C, device="cuda"))                          # the raw accumulators
    want = _linear(p, p["a"], p["cs"])
    wsb = _wsb(p)
    ws_a, ws_n = (torch.zeros(wsb, dtype=torch.uint8, device="cuda") for _ in range(2))
    out_a = torch.full((R, C), float("nan"), device="cuda")
    _lib.check(lib.gkg_affine_knn_prep(acc.data_ptr(), p["a"].data_ptr(), p["cs"].data_ptr(), *_run_args(p, out_a, C, ws_a), None),
               "gkg_affine_knn_prep")
    out_n = torch.full((R, C), float("nan"), device="cuda")
    scratch = _scratch(p)
    _lib.check(_fused(p, out_n, C, ws_n, scratch), "gkg_linear_bf16_knn_prep")
    torch.cuda.synchronize()
    assert torch.equal(out_n.view(torch.int32), want.view(torch.int32)), name
    assert torch.equal(out_a.view(torch.int32), want.view(torch.int32)), name
    print(f"{name}: workspace {wsb} bytes, {int((ws_a != 0).sum())} non-zero")
    assert int((ws_a != 0).sum()) > R * c                                          # the reference did prepare something
    assert torch.equal(ws_a, ws_n), (name, int((ws_a != ws_n).sum()))
    assert int(scratch.abs().sum()) == 0
    # the graphs: prepared call on the new workspace == unprepared call on `out` == the C oracle on `out`
    g_prep = _graph(p, out_n, ws_n, True)
    g_own = _graph(p, out_n, torch.zeros(wsb, dtype=torch.uint8, device="cuda"), False)
    torch.cuda.synchronize()
    assert torch.equal(g_prep, g_own), name

    def cm(t):
        return np.ascontiguousarray(t.reshape(t.shape[0], t.shape[1], G, c).permute(0, 2, 3, 1).reshape(-1, c, t.shape[1]).cpu().numpy())
    ref, _ = O.knn(cm(out_n.view(B, N, C)), None if p["y"] is None else cm(p["y"]), None if p["rp"] is None else p["rp"].cpu().numpy(),
                   p["k"], p["d"])
    assert np.array_equal(g_prep.cpu().numpy().view(np.uint16).astype(np.int64), ref), name


def test_two_runs_on_one_scratch_give_identical_bits_and_leave_it_zero():
    from gkgnet_amd import _lib
    p = _problem("1-straddle")
    scratch = _scratch(p)
    res = []
    for _ in range(2):
        ws = torch.zeros(_wsb(p), dtype=torch.uint8, device="cuda")
        out = torch.full((p["R"], p["C"]), float("nan"), device="cuda")
        _lib.check(_fused(p, out, p["C"], ws, scratch), "gkg_linear_bf16_knn_prep")
        torch.cuda.synchronize()
        assert int(scratch.abs().sum()) == 0
        res.append((out, ws))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("name", ["1-straddle", "8-pf-tiles"])
def test_output_pitch_inside_a_guard(name):
    """`out` with a row pitch above G c inside a sentinel-filled guard, x as a column slice of a wider tensor: the guard keeps its
    bits, the payload and the workspace are the packed call's."""
    from gkgnet_amd import _lib
    p = _problem(name)
    R, C, cin = p["R"], p["C"], p["cin"]
    ws0, ws1 = (torch.zeros(_wsb(p), dtype=torch.uint8, device="cuda") for _ in range(2))
    packed = torch.empty(R, C, device="cuda")
    _lib.check(_fused(p, packed, C, ws0, _scratch(p)), "gkg_linear_bf16_knn_prep")
    xw = torch.full((R, cin + 16), 7.0, device="cuda", dtype=BF16)
    xw[:, 8:8 + cin] = p["x"]
    guard = torch.full((R + 2, C + 8), S32, device="cuda", dtype=torch.int32)
    scratch = _scratch(p)
    _lib.check(_fused(p, guard, C + 8, ws1, scratch, x=xw[:, 8:]), "gkg_linear_bf16_knn_prep")
    torch.cuda.synchronize()
    assert torch.equal(guard[:R, :C], packed.view(torch.int32))
    assert bool((guard[R:] == S32).all()) and bool((guard[:, C:] == S32).all())
    assert torch.equal(ws0, ws1) and int(scratch.abs().sum()) == 0


@pytest.mark.parametrize("what", ["as_keys", "ochunk", "c6", "cin12", "bf16_contract"])
def test_unsupported_arguments_launch_nothing(what):
    from gkgnet_amd import _lib
    p = dict(_problem("7-small"))
    kw, cin = {}, None
    if what == "as_keys":
        kw = dict(as_keys=1)
    elif what == "ochunk":
        kw = dict(ochunk=p["C"] // 4)
    elif what == "c6":
        p.update(G=4, c=6, C=24)                    # G c = 24 passes the projection's cout % 8: the group width is what fails
    elif what == "cin12":
        cin = 12
    else:
        p["flags"] = p["flags"] | _lib.KNN_BF16_CONTRACT
    out = torch.full((p["R"], 2 * 80), S32, device="cuda", dtype=torch.int32)
    ws = torch.full((_wsb(_problem("7-small")),), 0x5A, dtype=torch.uint8, device="cuda")
    scratch = _scratch(p)
    rc = _fused(p, out, 2 * 80, ws, scratch, cin=cin, **kw)
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED, (what, rc)
    assert bool((out == S32).all()) and bool((ws == 0x5A).all()) and int(scratch.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ dispatch from the blocks
def _blocks(r):
    from gkgnet_amd import layers
    from gkgnet_amd.backbone import FFN
    from gkgnet_amd.grapher import Grapher
    from tests.util import keyed_fill_
    layers.norm_cfg["type"] = "BN"
    torch.manual_seed(0)
    C, G, H = 160, 2, 16
    g = Grapher(C, 9, 2, "mr", "gelu", "batch", True, False, 0.2, r, n=H * H, drop_path=0.0, relative_pos=True,
                use_multi_group=True, num_group=G)
    ffn = FFN(C, 4 * C, act="gelu")
    for m in (g, ffn):
        sd = m.state_dict()
        keyed_fill_(sd)
        m.load_state_dict(sd)
        m.cuda().eval()
    x = torch.randn(2, C, H, H, device="cuda").to(memory_format=torch.channels_last)
    return g, ffn, x


def _instrument(monkeypatch):
    """Counts of the two host functions of linear_bf16.py as ``fused`` calls them, and the flag word of every k-NN call."""
    from gkgnet_amd import _lib, fused
    counts, flags = {"eval": 0, "prep": 0}, []
    for key, name in (("eval", "linear_bf16_eval"), ("prep", "linear_bf16_knn_prep_eval")):
        def counted(*a, _real=getattr(fused, name), _key=key, **k):
            counts[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(fused, name, counted)
    lib = _lib.load()
    for name, pos in (("gkg_knn_fwd_tm16", 14), ("gkg_knn_fwd_tm", 15)):         # the position of `flags` (include/gkg_hip.h)
        def recording(*a, _real=getattr(lib, name), _pos=pos):
            flags.append(int(a[_pos]))
            return _real(*a)
        monkeypatch.setattr(lib, name, recording)
    return counts, flags


def _forward(g, ffn, x):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        return ffn(g(x))


@pytest.mark.parametrize("r", [2, 1])
def test_block_dispatch_prepares_the_queries_in_fc1_and_keeps_the_bits(r, monkeypatch):
    from gkgnet_amd import _lib, fused
    g, ffn, x = _blocks(r)
    counts, flags = _instrument(monkeypatch)
    outs = {}
    for lin, prep, knn_bf16 in [(False, False, False), (True, False, False), (True, True, False), (False, True, False),
                                (True, False, True), (True, True, True)]:
        monkeypatch.setattr(fused, "LIN_BF16", lin)
        monkeypatch.setattr(fused, "LIN_BF16_PREP", "all" if prep else False)      # "all": without the measured per-shape rule
        monkeypatch.setattr(fused, "KNN_BF16", knn_bf16)
        counts.update(eval=0, prep=0)
        flags.clear()
        outs[(lin, prep, knn_bf16)] = _forward(g, ffn, x)
        torch.cuda.synchronize()
        n_prepared = sum(1 for f in flags if f & _lib.KNN_X_PREPARED)
        assert len(flags) == 1
        if lin and prep and not knn_bf16:
            assert (counts["eval"], counts["prep"], n_prepared) == (3, 1, 1)
        else:
            assert (counts["eval"], counts["prep"], n_prepared) == (4 if lin else 0, 0, 0)
    assert torch.equal(outs[(True, True, False)], outs[(True, False, False)])     # both switches: the bits of lin_bf16 alone
    assert torch.equal(outs[(False, True, False)], outs[(False, False, False)])   # lin_bf16_prep alone: nothing changes
    assert torch.equal(outs[(True, True, True)], outs[(True, False, True)])       # the bf16 contraction keeps its path


def test_measured_rule_keeps_small_blocks_on_the_two_launches(monkeypatch):
    """LIN_BF16_PREP == True (GKG_ENABLE=lin_bf16_prep) applies linear_bf16.prep_pays: the 512-row test block is far outside it."""
    from gkgnet_amd import _lib, fused
    g, ffn, x = _blocks(2)
    counts, flags = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "LIN_BF16", True)
    monkeypatch.setattr(fused, "LIN_BF16_PREP", False)
    want = _forward(g, ffn, x)
    counts.update(eval=0, prep=0)
    flags.clear()
    monkeypatch.setattr(fused, "LIN_BF16_PREP", True)
    got = _forward(g, ffn, x)
    assert (counts["eval"], counts["prep"]) == (4, 0) and not any(f & _lib.KNN_X_PREPARED for f in flags)
    assert torch.equal(got, want)


def test_backbone_logits_identical_and_every_grapher_graph_prepared(monkeypatch):
    import os
    os.environ["GKG_RELPOS_DEVICE"] = "cuda"
    from gkgnet_amd import _lib, fused, layers
    from gkgnet_amd.backbone import GKGNet
    from gkgnet_amd.grapher import Grapher
    layers.norm_cfg["type"] = "BN"
    torch.manual_seed(0)
    net = GKGNet(choice="s", k=9, k_label_gcn=9, n_classes=80, size=576, num_group=2).cuda().eval()
    n_grapher = sum(1 for m in net.modules() if type(m) is Grapher)
    assert n_grapher >= 8
    img = torch.randn(1, 3, 576, 576, device="cuda")
    counts, flags = _instrument(monkeypatch)
    lib = _lib.load()
    inside = []                                     # k-NN flag words of the calls a Grapher (not a GrapherLabel) makes
    real_gf = fused.grapher_forward

    def grapher_forward(*a, **k):
        n0 = len(flags)
        res = real_gf(*a, **k)
        inside.extend(flags[n0:])
        return res
    monkeypatch.setattr(fused, "grapher_forward", grapher_forward)
    monkeypatch.setattr(fused, "LIN_BF16", True)
    res = {}
    for prep in (False, True):
        monkeypatch.setattr(fused, "LIN_BF16_PREP", "all" if prep else False)      # "all": without the measured per-shape rule
        counts.update(eval=0, prep=0)
        flags.clear()
        inside.clear()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            labels, gap, edge = net(img)
        torch.cuda.synchronize()
        res[prep] = (labels, gap, edge)
        assert len(inside) == n_grapher, (len(inside), n_grapher)
        prepared = [bool(f & _lib.KNN_X_PREPARED) for f in inside]
        assert all(prepared) if prep else not any(prepared), prepared
        assert counts["prep"] == (n_grapher if prep else 0)
    for u, v in zip(res[False], res[True]):
        assert u.dtype == v.dtype and torch.equal(u, v)
    assert lib is _lib.load()
