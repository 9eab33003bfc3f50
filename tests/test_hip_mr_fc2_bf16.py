"""gkg_mr_fc2_bf16 (csrc/gkg_mr_fc2_bf16.hip): the second half of a Grapher under bf16 inference — max-relative aggregation + grouped
1x1 projection + BN + GELU (reference torch_vertex.py:47-62, torch_nn.py:57-69), then fc2 + BN + residual (torch_vertex.py:325-333) —
as one launch that keeps the (T, 2C) bf16 matrix on chip, and its dispatch from ``fused.grapher_forward`` under
GKG_ENABLE=lin_bf16,mr_fc2_bf16.

The contract is bit identity with the two launches it replaces, gkg_mr_linear_bf16[_nn16] -> gkg_linear_bf16 (one definition of the
gather, the clamp, the GELU and the hidden's rounding; same contraction order on the same MFMA; the second launch's epilogue):
``torch.equal`` on the integer views, no tolerance.  Independently of the second kernel, the outputs are held to fc2's definition in
fp64 on the first launch's bf16 matrix, with the derived bounds of tests/test_hip_linear_bf16.py."""
import functools
import itertools

import pytest
import torch

from tests.test_hip_linear_bf16 import BF16, UNSUPPORTED, _TorchProxy, _call, _check, _definition, _planes

pytestmark = pytest.mark.gpu

# (B, G, C, N, M | None, k), each the smallest at which one thing can go wrong:
SHAPES = [(1, 2, 16, 64, None, 3),        # one full tile, co = 8 (both paddings), the generic-k path
          (2, 2, 80, 150, None, 9),       # co = 40: fc2's steps straddle conv groups; tiles straddle images; a partial last tile
          (3, 2, 160, 100, 25, 9),        # pooled keys, the stage-2 width of GKGNet-576
          (2, 8, 192, 333, 90, 18),       # the widest, G = 8, k = 18: the LDS-heaviest case
          (2, 1, 48, 65, None, 5),        # G = 1, co = 24, one token in the second tile
          (2, 3, 96, 100, None, 9),       # a conv group straddles two k-NN groups
          (1, 8, 96, 1100, 250, 18),      # 18 tiles: every XCD and a tail; the stage-1 width of pvig_m
          (1, 2, 160, 70, None, 4)]       # the wide tile form (C > 128) on the generic-k path
FULL = [(2, 2, 80, 150, None, 9), (2, 8, 192, 333, 90, 18)]
MODEL = (True, True, 1, "both")           # a2 given, residual, GELU, both outputs
S32, S16 = 0x7FC12345, 0x7FD5             # NaN patterns no kernel writes


@functools.lru_cache(maxsize=None)
def _problem(B, G, C, N, M, k):
    from gkgnet_amd import derived
    g = torch.Generator().manual_seed(11 + 1000 * C + 10 * N + k + B + 7 * G)
    Mk = N if M is None else M
    x = torch.randn(B, N, C, generator=g)
    src = None if M is None else torch.randn(B, Mk, C, generator=g)
    idx = torch.randint(0, Mk, (B * G, N, k), generator=g)
    conv = torch.nn.Conv2d(2 * C, 2 * C, 1, groups=4)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (C / 2) ** 0.5)
    conv = conv.cuda()
    w2 = (torch.randn(C, 2 * C, generator=g) / (2 * C) ** 0.5).to(BF16)
    a1, c1 = torch.rand(2 * C, generator=g) + 0.5, torch.randn(2 * C, generator=g) * 0.2
    a2, c2 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    res = torch.randn(B * N, C, generator=g)
    x, idx, w2, a1, c1, a2, c2, res = (t.cuda() for t in (x, idx, w2, a1, c1, a2, c2, res))
    src = None if src is None else src.cuda()
    idx16 = idx.to(torch.int16)                      # M <= 65536 in every shape: the bits of the u16 rows
    return dict(x=x, src=src, idx=idx, idx16=idx16, p1=derived.mr_planes(conv), conv=conv, w2=w2, p2=_planes(w2), a1=a1, c1=c1, a2=a2,
                c2=c2, res=res, T=B * N, M=Mk)


def _outs(T, C, outs):
    o32 = torch.empty(T, C, device="cuda") if outs in ("f32", "both") else None
    o16 = torch.empty(T, C, device="cuda", dtype=BF16) if outs in ("bf16", "both") else None
    return o32, o16


def _mr_call(shape, p, idx, h16, act):
    """The first of the two launches: -> rc, h16 (T, 2C) written."""
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    B, G, C, N, _, k = shape
    lib = _lib.load()
    fn = lib.gkg_mr_linear_bf16_nn16 if idx.dtype == torch.int16 else lib.gkg_mr_linear_bf16
    rc = fn(_ptr(p["x"]), _ptr(p["src"]), _ptr(idx), _ptr(p["p1"]), _ptr(p["a1"]), _ptr(p["c1"]), _ptr(h16), 2 * C, B, G, C // G, N,
            p["M"], k, act, _stream())
    torch.cuda.synchronize()
    return rc


def _fc2_call(shape, p, idx, a2, res, ldr, o32, ldo32, o16, ldo16, act, C=None):
    from gkgnet_amd import _lib
    from gkgnet_amd.ops import _ptr, _stream
    B, G, C0, N, _, k = shape
    C = C0 if C is None else C
    lib = _lib.load()
    fn = lib.gkg_mr_fc2_bf16_nn16 if idx.dtype == torch.int16 else lib.gkg_mr_fc2_bf16
    rc = fn(_ptr(p["x"]), _ptr(p["src"]), _ptr(idx), _ptr(p["p1"]), _ptr(p["a1"]), _ptr(p["c1"]), _ptr(p["p2"]), _ptr(a2), _ptr(p["c2"]),
            _ptr(res), ldr, _ptr(o32), ldo32, _ptr(o16), ldo16, B, G, C // G, N, p["M"], k, act, _stream())
    torch.cuda.synchronize()
    return rc


@functools.lru_cache(maxsize=None)
def _pair(shape, lists, has_a2, has_res, act, outs):
    """The two existing launches -> (h16, out_f32 | None, out_bf16 | None); computed once per form, never modified."""
    p = _problem(*shape)
    C, T = shape[2], p["T"]
    h16 = torch.empty(T, 2 * C, device="cuda", dtype=BF16)
    assert _mr_call(shape, p, p[lists], h16, act) == 0
    o32, o16 = _outs(T, C, outs)
    assert _call(h16, 2 * C, p["p2"], p["a2"] if has_a2 else None, p["c2"], p["res"] if has_res else None, C, o32, C, o16, C, T, 2 * C,
                 C, 0) == 0
    return h16, o32, o16


def _fused(shape, lists, has_a2, has_res, act, outs):
    p = _problem(*shape)
    C, T = shape[2], p["T"]
    o32, o16 = _outs(T, C, outs)
    rc = _fc2_call(shape, p, p[lists], p["a2"] if has_a2 else None, p["res"] if has_res else None, C, o32, C, o16, C, act)
    assert rc == 0
    return o32, o16


def _same_bits(got, want, what):
    for g, w, iv in zip(got, want, (torch.int32, torch.int16)):
        assert (g is None) == (w is None), what
        if g is not None:
            differ = int((g.view(iv) != w.view(iv)).sum())
            print(f"{what}: {g.dtype} elements that differ from the two launches: {differ} of {g.numel()}")
            assert torch.equal(g.view(iv), w.view(iv)), (what, differ)


@pytest.mark.parametrize("lists", ["idx", "idx16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bits_of_the_two_launches_in_the_form_the_model_uses(shape, lists):
    _same_bits(_fused(shape, lists, *MODEL), _pair(shape, lists, *MODEL)[1:], f"{shape} {lists} model form")


@pytest.mark.parametrize("has_a2,has_res,act,outs", list(itertools.product((True, False), (True, False), (0, 1), ("f32", "bf16", "both"))))
@pytest.mark.parametrize("shape", FULL, ids=str)
def test_bits_of_the_two_launches_in_every_form(shape, has_a2, has_res, act, outs):
    form = (has_a2, has_res, act, outs)
    _same_bits(_fused(shape, "idx16", *form), _pair(shape, "idx16", *form)[1:], f"{shape} a2={has_a2} res={has_res} act={act} {outs}")


def test_out_of_range_index_entries_are_clamped_as_in_the_pair():
    shape = (2, 2, 80, 150, None, 9)
    p = dict(_problem(*shape))
    g = torch.Generator().manual_seed(5)
    idx = p["idx"].clone()
    where = torch.rand(idx.shape, generator=g).cuda()
    idx[where < 0.05] = -1
    idx[where > 0.95] = p["M"]
    assert int((idx < 0).sum()) > 0 and int((idx >= p["M"]).sum()) > 0
    C, T = shape[2], p["T"]
    h16 = torch.empty(T, 2 * C, device="cuda", dtype=BF16)
    assert _mr_call(shape, p, idx, h16, 1) == 0
    w32, w16 = _outs(T, C, "both")
    assert _call(h16, 2 * C, p["p2"], p["a2"], p["c2"], p["res"], C, w32, C, w16, C, T, 2 * C, C, 0) == 0
    o32, o16 = _outs(T, C, "both")
    assert _fc2_call(shape, p, idx, p["a2"], p["res"], C, o32, C, o16, C, 1) == 0
    _same_bits((o32, o16), (w32, w16), f"{shape} with clamped entries")


@pytest.mark.parametrize("shape", [(2, 2, 80, 150, None, 9), (3, 2, 160, 100, 25, 9), (2, 8, 192, 333, 90, 18)], ids=str)
def test_outputs_hold_fc2s_definition_on_the_first_launchs_matrix(shape):
    """Independent of the second kernel: the (T, 2C) matrix of the FIRST launch as given operands, fc2's contract in fp64."""
    p = _problem(*shape)
    C = shape[2]
    h16 = _pair(shape, "idx16", *MODEL)[0]
    hd, wd = h16.double().cpu(), p["w2"].double().cpu()
    want, bound = _definition(hd @ wd.t(), hd.abs() @ wd.abs().t(), 2 * C, p["a2"].cpu(), p["c2"].cpu(), p["res"].cpu(), 0)
    o32, o16 = _fused(shape, "idx16", *MODEL)
    _check(o32, o16, want, bound, f"{shape} against fc2's definition")


@pytest.mark.parametrize("shape", [(2, 2, 80, 150, None, 9), (2, 8, 192, 333, 90, 18), (1, 8, 96, 1100, 250, 18)], ids=str)
def test_pitches_and_bounds(shape):
    """Row pitches above the widths, the residual a column slice of a wider tensor, outputs inside sentinel-filled guards: the guards
    keep their bits and the payload equals the dense call's."""
    p = _problem(*shape)
    C, T = shape[2], p["T"]
    d32, d16 = _fused(shape, "idx16", *MODEL)
    rw = torch.full((T, C + 12), 3.0, device="cuda")
    rw[:, 4:4 + C] = p["res"]
    g32 = torch.full((T + 2, C + 8), S32, device="cuda", dtype=torch.int32)
    g16 = torch.full((T + 2, C + 8), S16, device="cuda", dtype=torch.int16)
    rc = _fc2_call(shape, p, p["idx16"], p["a2"], rw[:, 4:], C + 12, g32, C + 8, g16, C + 8, 1)
    assert rc == 0
    assert torch.equal(g32[:T, :C], d32.view(torch.int32)) and torch.equal(g16[:T, :C], d16.view(torch.int16))
    assert bool((g32[T:] == S32).all()) and bool((g32[:, C:] == S32).all())
    assert bool((g16[T:] == S16).all()) and bool((g16[:, C:] == S16).all())


@pytest.mark.parametrize("case", ["C=208", "ldo16=C+4"])
def test_unsupported_problems_launch_nothing(case):
    from gkgnet_amd import _lib
    shape = (2, 2, 80, 150, None, 9)
    p = _problem(*shape)
    T, W = p["T"], 256
    g32 = torch.full((T, W), S32, device="cuda", dtype=torch.int32)
    g16 = torch.full((T, W), S16, device="cuda", dtype=torch.int16)
    res = torch.zeros(T, W, device="cuda")
    if case == "C=208":
        # the operands are large enough for any width: the library must refuse before it reads or writes anything
        assert _lib.load().gkg_mr_fc2_bf16_supported(2, 2, 104, 150, 150, 9, 1, 1, 1, 1) == 0
        big = dict(p, x=torch.zeros(2, 150, 208, device="cuda"), p1=torch.zeros(1 << 16, device="cuda", dtype=BF16),
                   p2=torch.zeros(1 << 17, device="cuda", dtype=BF16), a1=torch.ones(416, device="cuda"), c1=torch.ones(416, device="cuda"),
                   c2=torch.ones(208, device="cuda"))
        rc = _fc2_call(shape, big, p["idx16"], torch.ones(208, device="cuda"), res, W, g32, W, g16, W, 1, C=208)
    else:
        rc = _fc2_call(shape, p, p["idx16"], p["a2"], res, W, g32, W, g16, 80 + 4, 1)
    assert rc == UNSUPPORTED == _lib.ERR_UNSUPPORTED
    assert bool((g32 == S32).all()) and bool((g16 == S16).all())      # the NaN-filled outputs stay all-NaN


def test_two_calls_give_identical_bits():
    shape = (2, 8, 192, 333, 90, 18)
    a, b = _fused(shape, "idx16", *MODEL), _fused(shape, "idx16", *MODEL)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))


# ------------------------------------------------------------------------------------------------ dispatch from the blocks
def _blocks():
    from gkgnet_amd import layers
    from gkgnet_amd.backbone import FFN
    from gkgnet_amd.grapher import Grapher, GrapherLabel
    from tests.util import keyed_fill_
    layers.norm_cfg["type"] = "BN"
    torch.manual_seed(0)
    C, G, H, L = 160, 2, 16, 80
    g = Grapher(C, 9, 2, "mr", "gelu", "batch", True, False, 0.2, 2, n=H * H, drop_path=0.0, relative_pos=True,
                use_multi_group=True, num_group=G)
    ffn = FFN(C, 4 * C, act="gelu")
    wide = Grapher(640, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=36, drop_path=0.0, relative_pos=True,
                   use_multi_group=True, num_group=G)
    gl = GrapherLabel(C, 9, 1, "mr", "gelu", "batch", True, False, 0.2, 1, n=H * H, drop_path=0.0, relative_pos=False,
                      num_nodes=L, use_multi_group=True, num_group=G)
    for m in (g, ffn, wide, gl):
        sd = m.state_dict()
        keyed_fill_(sd)
        m.load_state_dict(sd)
        m.cuda().eval()
    x = torch.randn(2, C, H, H, device="cuda")
    e = torch.randn(2, L, C, device="cuda")
    return g, ffn, wide, gl, x, e


def _instrument(monkeypatch):
    """Counting wrappers around linear_bf16_eval, mr_grouped_linear_eval and mr_fc2_bf16_eval, the two affine entry points and the
    library GEMMs of ``fused``."""
    from gkgnet_amd import _lib, fused
    calls, counts = {"lin": 0, "mr": 0, "tail": 0}, {}
    for key, name in (("lin", "linear_bf16_eval"), ("mr", "mr_grouped_linear_eval"), ("tail", "mr_fc2_bf16_eval")):
        def counting(*a, _real=getattr(fused, name), _key=key, **k):
            calls[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(fused, name, counting)
    lib = _lib.load()
    for name in ("gkg_affine_act", "gkg_affine_act_dual"):
        def counted(*a, _real=getattr(lib, name), _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    monkeypatch.setattr(fused, "torch", _TorchProxy(counts))
    return calls, counts


def _reset(calls, counts):
    calls.update(lin=0, mr=0, tail=0)
    counts.clear()


NO_LIBRARY_GEMM = ("mm", "addmm", "_addmm_activation", "gkg_affine_act", "gkg_affine_act_dual")


def test_block_dispatch_runs_the_tail_as_one_launch_with_the_pairs_bits(monkeypatch):
    """Grapher + FFN on the channels-last chain, eval, bf16 autocast, gradients off, LIN_BF16 on."""
    from gkgnet_amd import fused
    g, ffn, _, _, x, _ = _blocks()
    xcl = x.to(memory_format=torch.channels_last)
    calls, counts = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "LIN_BF16", True)
    got = {}
    for on in (False, "all"):
        monkeypatch.setattr(fused, "MR_FC2_BF16", on)
        _reset(calls, counts)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            y = g(xcl)
            assert (calls["tail"], calls["mr"], calls["lin"]) == ((1, 0, 1) if on else (0, 1, 2)), calls      # the Grapher: fc1 (+ fc2)
            o = ffn(y)
        assert all(counts.get(n, 0) == 0 for n in NO_LIBRARY_GEMM), counts
        outs = []
        for t in (y, o):
            assert t.dtype == torch.float32 and t.shape == x.shape and fused.is_channels_last(t)
            ent = getattr(t, "_gkg_bf16", None)
            assert ent is not None and ent[0] == t._version and ent[1].dtype == BF16
            outs += [t, ent[1]]
        got[on] = outs
    for t_off, t_on in zip(got[False], got["all"]):
        iv = torch.int32 if t_off.dtype == torch.float32 else torch.int16
        assert torch.equal(t_on.view(iv), t_off.view(iv))
    # ... and with the graph asked for (int64 lists): the same, with equal edge lists
    rp = g._get_relative_pos(g.relative_pos, 16, 16)
    for on in (False, "all"):
        monkeypatch.setattr(fused, "MR_FC2_BF16", on)
        _reset(calls, counts)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            y, edge = fused.grapher_forward(g, xcl, rp, g.graph_conv.num_head, want_edge=True)
        assert (calls["tail"], calls["mr"], calls["lin"]) == ((1, 0, 1) if on else (0, 1, 2)), calls
        assert all(counts.get(n, 0) == 0 for n in NO_LIBRARY_GEMM), counts
        assert edge is not None and edge.dtype == torch.int64
        got[on] = (y, y._gkg_bf16[1], edge)
    assert torch.equal(got["all"][0].view(torch.int32), got[False][0].view(torch.int32))
    assert torch.equal(got["all"][1].view(torch.int16), got[False][1].view(torch.int16))
    assert torch.equal(got["all"][2], got[False][2])


def test_forms_outside_the_dispatch_keep_their_path_bit_for_bit(monkeypatch):
    """A Grapher wider than the envelope, an NCHW-contiguous input, a GrapherLabel and MR_GEMM off make no mr_fc2_bf16_eval call with
    the switch on and return the switch-off bits."""
    from gkgnet_amd import fused
    g, _, wide, gl, x, e = _blocks()
    calls, counts = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "LIN_BF16", True)
    feats = x.to(memory_format=torch.channels_last)
    xw = torch.randn(2, 640, 6, 6, device="cuda").to(memory_format=torch.channels_last)
    got = {}
    for on in (False, "all"):
        monkeypatch.setattr(fused, "MR_FC2_BF16", on)
        _reset(calls, counts)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            o_wide = wide(xw)
            assert (calls["mr"], calls["lin"]) == (1, 2), calls     # the pair, on the own kernels
            o_nchw = g(x)
            e2, idx = gl(e, feats)
            monkeypatch.setattr(fused, "MR_GEMM", False)
            o_nomr = g(feats)
            monkeypatch.setattr(fused, "MR_GEMM", True)
        assert calls["tail"] == 0, calls
        got[on] = (o_wide, o_nchw, e2, idx, o_nomr)
    for t_off, t_on in zip(got[False], got["all"]):
        assert t_off.dtype == t_on.dtype and torch.equal(t_off, t_on)


def test_whole_network_keeps_its_bits_and_fuses_every_narrow_grapher(monkeypatch):
    """The tiny backbone of tests/test_backbone.py (fixture F10) on a channels-last image, eval, bf16 autocast, gradients off."""
    from gkgnet_amd import fused, layers
    from gkgnet_amd.backbone import GKGNet
    from gkgnet_amd.grapher import Grapher
    from tests.util import keyed_fill_, load_fixture
    layers.norm_cfg["type"] = "BN"
    meta, a = load_fixture("f10_backbone_tiny")
    net = GKGNet(**meta["ctor"])
    sd = net.state_dict()
    with torch.no_grad():
        keyed_fill_(sd, seed=10)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    img = torch.from_numpy(a["img"]).cuda().to(memory_format=torch.channels_last)
    narrow = sum(1 for m in net.backbone.modules() if isinstance(m, Grapher) and m.channels <= 192)
    assert narrow >= 1
    calls, _ = _instrument(monkeypatch)
    monkeypatch.setattr(fused, "LIN_BF16", True)
    got = {}
    for on in (False, "all"):
        monkeypatch.setattr(fused, "MR_FC2_BF16", on)
        _reset(calls, {})
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            got[on] = net(img)
        assert calls["tail"] == (narrow if on else 0), (calls, narrow)
    for t_off, t_on in zip(got[False], got["all"]):
        assert t_off.dtype == t_on.dtype and torch.equal(t_off, t_on)
