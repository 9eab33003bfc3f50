"""gkgnet_amd/derived.py on the CPU: the one staleness protocol behind the six parameter-derived caches (bf16 weight copy, BN-folded
weight and shifts, the three fragment arrays, an eval-mode BN's (a, c)), the one fragment builder and the fold."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

BF16 = torch.bfloat16
CIN, COUT = 16, 32
SLOTS = ("w16", "folded", "lin_planes", "lin_planes_t", "mr_planes", "eval_ac")
STATS_SLOTS = ("folded", "eval_ac")


class _AffineLib:
    """Stands in for the library where the device kernel would run: gkg_bn_eval_affine computed by torch on the host buffers behind
    the pointers it is handed, and counted."""

    def __init__(self):
        self.calls = 0

    def gkg_bn_eval_affine(self, w, b, bias, mean, var, a, c, n, eps, stream):
        def f32(ptr):
            return None if ptr is None else torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(ptr)))
        self.calls += 1
        a_, c_ = _affine(f32(w), f32(b), f32(bias), f32(mean), f32(var), eps)
        f32(a).copy_(a_)
        f32(c).copy_(c_)
        return 0


def _affine(w, b, bias, mean, var, eps):
    a = w * torch.rsqrt(var + eps)
    c = b - a * mean
    return a, (c if bias is None else c + a * bias)


@pytest.fixture
def lib(monkeypatch):
    from gkgnet_amd import bn_passes, derived
    monkeypatch.setattr(bn_passes, "_stream", lambda: 0)
    derived.clear()
    yield _AffineLib()
    derived.clear()


def _layer(slot, guarded=True, bias=True, seed=0):
    from gkgnet_amd import layers
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(32, 32, 1, groups=4, bias=bias) if slot == "mr_planes" else torch.nn.Conv2d(CIN, COUT, 1, bias=bias)
    bn = (layers.GuardedBatchNorm2d if guarded else torch.nn.BatchNorm2d)(conv.out_channels).eval()
    with torch.no_grad():
        bn.weight.normal_(1.0, 0.2)
        bn.bias.normal_()
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
    return conv, bn


def _owner(slot, conv, bn):
    return bn if slot == "eval_ac" else conv


def _call(slot, conv, bn, lib):
    from gkgnet_amd import bn_passes, derived
    with torch.no_grad():
        if slot == "eval_ac":
            return bn_passes.eval_ac(lib, bn, conv.bias, conv.out_channels)
        if slot == "folded":
            return derived.folded(conv, bn)
        if slot == "lin_planes_t":
            return derived.lin_planes(conv, transposed=True)
        return getattr(derived, slot)(conv)


def _ref_fragments(m, k_pad, n_pad):
    """The layout, index by index (include/gkg_hip.h): [k_pad / 8][n_pad][8], fragment (f, n) = m[n][8f .. 8f+7], zero outside."""
    n, k = m.shape
    p = torch.zeros(k_pad // 8, n_pad, 8, dtype=BF16)
    m16 = m.to(BF16)
    for f in range((k + 7) // 8):
        for j in range(n):
            p[f, j, :min(8, k - 8 * f)] = m16[j, 8 * f:8 * f + 8]
    return p


def _up(v, m):
    return (v + m - 1) // m * m


def _parent_fold(conv, bn):
    """The fold's arithmetic as fused.py spelled it (twice: weights + bf16 shift, fp32 shift) before the move, kept as the reference."""
    with torch.no_grad():
        a = bn.weight.float() * torch.rsqrt(bn.running_var.float() + bn.eps)
        shift = bn.bias.float() - a * bn.running_mean.float()
        if conv.bias is not None:
            shift = shift + a * conv.bias.float()
        wf = (conv.weight.float().view(conv.weight.shape[0], -1) * a.view(-1, 1)).to(BF16).contiguous()
        return wf, shift.to(BF16).contiguous(), shift.contiguous()


def _want(slot, conv, bn):
    """What the slot must hold for the CURRENT parameters, stated independently of derived.py."""
    w = conv.weight.detach()
    w2 = w.reshape(w.shape[0], -1)
    if slot == "w16":
        return (w.to(BF16),)
    if slot == "folded":
        return _parent_fold(conv, bn)
    if slot == "lin_planes":
        return (_ref_fragments(w2, _up(CIN, 16), _up(COUT, 32)),)
    if slot == "lin_planes_t":
        return (_ref_fragments(w2.t(), _up(COUT, 16), _up(CIN, 32)),)
    if slot == "mr_planes":
        return (torch.stack([_ref_fragments(g, 16, 32) for g in w2.reshape(4, 8, 8)]),)
    return _affine(bn.weight.detach(), bn.bias.detach(), None if conv.bias is None else conv.bias.detach(), bn.running_mean,
                   bn.running_var, bn.eps)


def _tup(v):
    return v if isinstance(v, tuple) else (v,)


def _same(got, want):
    got = _tup(got)
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want))


def _is(a, b):
    return all(x is y for x, y in zip(_tup(a), _tup(b)))


def _params(conv, bn):
    return [conv.weight, conv.bias, bn.weight, bn.bias]


def _update_data(conv, bn):
    from gkgnet_amd.planes import mark_parameters_updated
    for p in _params(conv, bn):
        p.data.mul_(1.5)
    mark_parameters_updated()


def _update_add(conv, bn):
    with torch.no_grad():
        for p in _params(conv, bn):
            p.add_(0.25)


def _update_fused_step(conv, bn):
    for p in _params(conv, bn):
        p.grad = torch.ones_like(p)
    try:
        opt = torch.optim.AdamW(_params(conv, bn), lr=0.5, fused=True)
    except RuntimeError as e:                     # a build without fused kernels for this device
        pytest.skip(str(e))
    opt.step()


@pytest.mark.parametrize("slot", SLOTS)
def test_second_call_returns_the_same_object(slot, lib):
    from gkgnet_amd import derived
    conv, bn = _layer(slot)
    v = _call(slot, conv, bn, lib)
    assert _same(v, _want(slot, conv, bn))
    assert _is(_call(slot, conv, bn, lib), v)
    assert _is(derived.peek(_owner(slot, conv, bn), slot), v)
    assert not any(k.startswith("_gkg_") and k != "_gkg_epoch" for m in (conv, bn) for k in vars(m))     # nothing hangs on the modules
    derived.clear(_owner(slot, conv, bn))
    assert derived.peek(_owner(slot, conv, bn), slot) is None


@pytest.mark.parametrize("update", [_update_data, _update_add, _update_fused_step], ids=["data_and_mark", "add_", "fused_step"])
@pytest.mark.parametrize("slot", SLOTS)
def test_rebuilt_after_a_parameter_update(slot, update, lib):
    conv, bn = _layer(slot)
    v0 = tuple(t.clone() for t in _tup(_call(slot, conv, bn, lib)))
    update(conv, bn)
    v1 = _call(slot, conv, bn, lib)
    assert _same(v1, _want(slot, conv, bn))
    assert not _same(v1, v0)


def _replace_weight(conv, bn, arr):
    conv.weight = torch.nn.Parameter(torch.from_numpy(arr))


def _replace_running_var(conv, bn, arr):
    bn.running_var = torch.from_numpy(arr)


def _replace_conv_bias(conv, bn, arr):
    conv.bias = torch.nn.Parameter(torch.from_numpy(arr))


REPLACED = [(s, _replace_weight) for s in SLOTS if s != "eval_ac"] + [(s, r) for s in STATS_SLOTS
                                                                      for r in (_replace_running_var, _replace_conv_bias)]


@pytest.mark.parametrize("slot,replace", REPLACED, ids=[f"{s}-{r.__name__[9:]}" for s, r in REPLACED])
def test_a_new_tensor_at_the_same_address_with_version_0_is_rebuilt(slot, replace, lib):
    """Same pointer, same version token, another tensor: the numpy array keeps the address, every torch.from_numpy tensor over it
    starts at version 0."""
    conv, bn = _layer(slot)
    like = {_replace_weight: conv.weight, _replace_running_var: bn.running_var, _replace_conv_bias: conv.bias}[replace]
    rng = np.random.default_rng(7)
    arr = rng.uniform(0.5, 2.0, size=tuple(like.shape)).astype(np.float32)
    replace(conv, bn, arr)
    v0 = tuple(t.clone() for t in _tup(_call(slot, conv, bn, lib)))
    assert _same(v0, _want(slot, conv, bn))
    old = {_replace_weight: conv.weight, _replace_running_var: bn.running_var, _replace_conv_bias: conv.bias}[replace]
    arr[:] = rng.uniform(0.5, 2.0, size=arr.shape).astype(np.float32)
    replace(conv, bn, arr)
    new = {_replace_weight: conv.weight, _replace_running_var: bn.running_var, _replace_conv_bias: conv.bias}[replace]
    assert new is not old and new.data_ptr() == old.data_ptr() and new._version == old._version == 0
    v1 = _call(slot, conv, bn, lib)
    assert _same(v1, _want(slot, conv, bn))
    assert not _same(v1, v0)


@pytest.mark.parametrize("slot", STATS_SLOTS)
def test_mode_switches_and_touch_invalidate_what_reads_the_statistics(slot, lib):
    from gkgnet_amd import bn_passes
    conv, bn = _layer(slot)
    v0 = _call(slot, conv, bn, lib)
    bn.train()
    bn.eval()
    v1 = _call(slot, conv, bn, lib)
    assert not _is(v1, v0) and _same(v1, _want(slot, conv, bn))
    bn.train()
    v2 = _call(slot, conv, bn, lib)
    assert not _is(v2, v1) and _is(_call(slot, conv, bn, lib), v2)
    assert bn_passes.touch(bn)                                   # a kernel is about to move the statistics through raw pointers
    bn.running_var.data.mul_(3.0)                                # ... like this: no counter moves
    v3 = _call(slot, conv, bn, lib)
    assert not _is(v3, v2) and _same(v3, _want(slot, conv, bn)) and not _same(v3, tuple(_tup(v2)))


@pytest.mark.parametrize("slot", STATS_SLOTS)
def test_a_plain_batchnorm_is_never_stored(slot, lib):
    from gkgnet_amd import derived
    conv, bn = _layer(slot, guarded=False)
    v0 = _call(slot, conv, bn, lib)
    v1 = _call(slot, conv, bn, lib)
    assert not _is(v1, v0) and _same(v1, _want(slot, conv, bn))
    assert derived.peek(_owner(slot, conv, bn), slot) is None


def test_eval_ac_with_gradients_on_builds_every_time_and_stores_nothing(lib):
    from gkgnet_amd import bn_passes, derived
    conv, bn = _layer("eval_ac")
    with torch.enable_grad():
        ac0 = bn_passes.eval_ac(lib, bn, conv.bias, COUT)
        ac1 = bn_passes.eval_ac(lib, bn, conv.bias, COUT)
    assert lib.calls == 2 and not _is(ac0, ac1) and _same(ac1, _want("eval_ac", conv, bn))
    assert derived.peek(bn, "eval_ac") is None
    with torch.no_grad():
        ac2 = bn_passes.eval_ac(lib, bn, conv.bias, COUT)
        ac3 = bn_passes.eval_ac(lib, bn, conv.bias, COUT)
    assert lib.calls == 3 and _is(ac2, ac3)
    with torch.no_grad():                                        # another length is another value
        bn_passes.eval_ac(lib, bn, conv.bias, COUT // 2)
    assert lib.calls == 4


def test_deepcopy_and_pickle_carry_no_cache(lib):
    from gkgnet_amd import derived
    conv, bn = _layer("w16")
    gconv, _ = _layer("mr_planes", seed=1)
    mod = torch.nn.Sequential(conv, bn, gconv)
    for slot in SLOTS:
        _call(slot, gconv if slot == "mr_planes" else conv, bn, lib)
    twin = copy.deepcopy(mod)
    back = pickle.loads(pickle.dumps(mod))
    for m in (twin, back):
        for slot in SLOTS:
            assert derived.peek(m[1] if slot == "eval_ac" else m[2] if slot == "mr_planes" else m[0], slot) is None, slot
    with torch.no_grad():
        for p in twin.parameters():
            p.mul_(-2.0)
    for slot in SLOTS:
        c = twin[2] if slot == "mr_planes" else twin[0]
        assert _same(_call(slot, c, twin[1], lib), _want(slot, c, twin[1])), slot
        o = gconv if slot == "mr_planes" else conv
        assert _same(_call(slot, o, bn, lib), _want(slot, o, bn)), slot                    # the original keeps its own


@pytest.mark.parametrize("k,n", [(8, 8), (40, 24), (72, 136)])
def test_bf16_fragments_bit_for_bit(k, n):
    from gkgnet_amd import _lib, derived
    lib = _lib.load()
    torch.manual_seed(k + n)
    w = torch.randn(n, k)
    k_pad, n_pad = _up(k, derived.K_ALIGN), _up(n, derived.N_ALIGN)
    assert (derived.K_ALIGN, derived.N_ALIGN) == (16, 32)
    p = derived.bf16_fragments(w, k_pad, n_pad)
    assert p.dtype == BF16 and p.is_contiguous() and tuple(p.shape) == (k_pad // 8, n_pad, 8)
    assert torch.equal(p.view(torch.int16), _ref_fragments(w, k_pad, n_pad).view(torch.int16))
    assert p.numel() * 2 == lib.gkg_linear_bf16_planes_bytes(k, n)
    conv = torch.nn.Conv2d(k, n, 1)
    conv.weight.data.copy_(w.view(n, k, 1, 1))
    assert torch.equal(derived.lin_planes(conv).view(torch.int16), p.view(torch.int16))


def test_bf16_fragments_of_the_transposed_weight():
    from gkgnet_amd import _lib, derived
    ci, co = 40, 24
    torch.manual_seed(9)
    conv = torch.nn.Conv2d(ci, co, 1)
    w = conv.weight.detach().reshape(co, ci)
    k_pad, n_pad = _up(co, 16), _up(ci, 32)                       # contraction cout, columns cin
    pt = derived.bf16_fragments(w.t(), k_pad, n_pad)
    assert tuple(pt.shape) == (4, 64, 8)
    assert torch.equal(pt.view(torch.int16), _ref_fragments(w.t(), k_pad, n_pad).view(torch.int16))
    assert pt.numel() * 2 == _lib.load().gkg_linear_bf16_planes_bytes(co, ci)
    assert torch.equal(derived.lin_planes(conv, transposed=True).view(torch.int16), pt.view(torch.int16))


@pytest.mark.parametrize("ci,co", [(8, 8), (24, 24), (24, 40)])
def test_bf16_fragments_of_a_stack_of_four(ci, co):
    """gkg_mr_linear_planes_bytes(C) describes the grouped layer's own weight, whose groups are square (co == ci == C / 2): the
    square stacks are checked against it (and through derived.mr_planes), the 24 x 40 stack against four dense arrays of the same
    paddings."""
    from gkgnet_amd import _lib, derived
    lib = _lib.load()
    torch.manual_seed(ci + co)
    w = torch.randn(4, co, ci)
    k_pad, n_pad = _up(ci, 16), _up(co, 32)
    p = derived.bf16_fragments(w, k_pad, n_pad)
    assert p.is_contiguous() and tuple(p.shape) == (4, k_pad // 8, n_pad, 8)
    for g in range(4):
        assert torch.equal(p[g].view(torch.int16), _ref_fragments(w[g], k_pad, n_pad).view(torch.int16)), g
    assert p.numel() * 2 == 4 * lib.gkg_linear_bf16_planes_bytes(ci, co)
    if ci == co:
        assert p.numel() * 2 == lib.gkg_mr_linear_planes_bytes(4 * ci // 2)
        conv = torch.nn.Conv2d(4 * ci, 4 * co, 1, groups=4)
        conv.weight.data.copy_(w.view(4 * co, ci, 1, 1))
        assert torch.equal(derived.mr_planes(conv).view(torch.int16), p.view(torch.int16))


@pytest.mark.parametrize("bias", [True, False])
def test_fold_equals_the_former_two_functions(bias, lib):
    from gkgnet_amd import derived
    conv, bn = _layer("folded", bias=bias)
    wf, c16, c32 = derived.folded(conv, bn)
    want = _parent_fold(conv, bn)
    assert wf.dtype == BF16 and c16.dtype == BF16 and c32.dtype == torch.float32 and tuple(wf.shape) == (COUT, CIN)
    assert torch.equal(wf, want[0]) and torch.equal(c16, want[1]) and torch.equal(c32, want[2])
