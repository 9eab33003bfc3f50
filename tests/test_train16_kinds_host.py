"""The table of element kinds behind GKG_ENABLE=train_bf16 / train_f16 (linear_bf16.KINDS) and the one decision that walks it
(fused._train_16bit), the parts that need no device: the rows, their entry points in the derived binding, derived's slot names
and which row each autocast dtype gets with the switches on and off."""
import types

import torch


def test_the_table_has_the_two_rows():
    from gkgnet_amd import linear_bf16
    assert list(linear_bf16.KINDS) == ["bf16", "f16"]
    assert linear_bf16.KINDS["bf16"] is linear_bf16.BF16 and linear_bf16.KINDS["f16"] is linear_bf16.F16
    for name, kind in linear_bf16.KINDS.items():
        assert kind.name == name
    assert (linear_bf16.BF16.autocast, linear_bf16.F16.autocast) == (torch.bfloat16, torch.float16)
    assert (linear_bf16.BF16.fragment, linear_bf16.F16.fragment) == (torch.bfloat16, torch.float16)


def test_every_entry_point_of_a_row_is_declared_in_the_header():
    from gkgnet_amd import _abi, _lib, linear_bf16
    protos = _abi.header().protos
    for kind in linear_bf16.KINDS.values():
        for name in (kind.f32a, kind.f32a_supported, kind.planes_bytes):
            assert name in protos and name in _lib.EXPORTS, (kind.name, name)
            assert ("_%s_" % kind.name) in name, (kind.name, name)
        assert protos[kind.f32a] == protos["gkg_linear_bf16_f32a"]
        assert protos[kind.f32a_supported] == protos["gkg_linear_bf16_f32a_supported"]
        assert protos[kind.planes_bytes] == protos["gkg_linear_bf16_planes_bytes"]


def test_the_four_slot_names_are_distinct_and_what_they_were():
    from gkgnet_amd import linear_bf16
    assert linear_bf16.BF16.slots == ("lin_planes", "lin_planes_t")
    assert linear_bf16.F16.slots == ("lin_planes_f16", "lin_planes_t_f16")
    slots = [s for kind in linear_bf16.KINDS.values() for s in kind.slots]
    assert len(slots) == 4 and len(set(slots)) == 4


def test_lin_planes_fills_the_row_s_slot_by_name_or_by_row():
    from gkgnet_amd import derived, linear_bf16
    conv = torch.nn.Conv2d(24, 40, 1)
    for kind in linear_bf16.KINDS.values():
        for transposed in (False, True):
            assert derived.peek(conv, kind.slots[transposed]) is None
            p = derived.lin_planes(conv, kind, transposed)
            assert p.dtype == kind.fragment and derived.peek(conv, kind.slots[transposed]) is p
            assert derived.lin_planes(conv, kind.name, transposed=transposed) is p
    assert derived.lin_planes(conv) is derived.peek(conv, "lin_planes")           # the inference callers' spelling: bf16, as it is


def test_only_bf16_owns_a_weight_gradient_kernel():
    from gkgnet_amd import linear_bf16
    assert {name: kind.own_wgrad for name, kind in linear_bf16.KINDS.items()} == {"bf16": True, "f16": False}


def _x():
    return types.SimpleNamespace(dtype=torch.float32, shape=(324, 80), is_cuda=True, stride=lambda d: (80, 1)[d])


def test_the_decision_returns_the_row_of_the_autocast_dtype(monkeypatch):
    """Plain Python objects: no CUDA tensor, no autocast context (the two torch queries are answered by the test)."""
    from gkgnet_amd import fused, linear_bf16
    auto = {"dtype": torch.bfloat16}
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: auto["dtype"])
    monkeypatch.setattr(fused, "DETERMINISTIC", False)
    bn = types.SimpleNamespace(training=True, track_running_stats=True)
    conv = types.SimpleNamespace(groups=1, weight=types.SimpleNamespace(shape=(160, 80, 1, 1)))
    x = _x()
    rows = ((torch.bfloat16, "TRAIN_BF16", linear_bf16.BF16), (torch.float16, "TRAIN_F16", linear_bf16.F16))
    with torch.enable_grad():
        monkeypatch.setattr(fused, "TRAIN_BF16", True)
        monkeypatch.setattr(fused, "TRAIN_F16", True)
        for dtype, _, kind in rows:
            auto["dtype"] = dtype
            got = fused._train_16bit(x, conv, bn)
            assert got is not None and got[0] is kind and got[1] is conv
        for dtype, switch, _ in rows:                                            # each kind's own switch off, the other's on
            monkeypatch.setattr(fused, "TRAIN_BF16", True)
            monkeypatch.setattr(fused, "TRAIN_F16", True)
            monkeypatch.setattr(fused, switch, False)
            auto["dtype"] = dtype
            assert fused._train_16bit(x, conv, bn) is None
        monkeypatch.setattr(fused, "TRAIN_BF16", True)
        monkeypatch.setattr(fused, "TRAIN_F16", True)
        monkeypatch.setattr(fused, "DETERMINISTIC", True)                        # own_wgrad is what GKG_DETERMINISTIC refuses
        auto["dtype"] = torch.bfloat16
        assert fused._train_16bit(x, conv, bn) is None
        auto["dtype"] = torch.float16
        assert fused._train_16bit(x, conv, bn)[0] is linear_bf16.F16
