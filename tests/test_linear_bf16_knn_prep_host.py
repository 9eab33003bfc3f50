"""gkg_linear_bf16_knn_prep (csrc/gkg_linear_bf16.hip: a Grapher's fc1 and the k-NN's token preparation in one launch), the parts
that need no device: the three entry points in the header and the derived binding, the pure host functions, the opt-in switch
and the dispatch predicate ``fused._lin`` asks."""
import ctypes as C
import types

import torch

I, U, P, F, Z = C.c_int, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t
NAMES = ("gkg_linear_bf16_knn_prep_scratch_bytes", "gkg_linear_bf16_knn_prep_supported", "gkg_linear_bf16_knn_prep")


def test_header_declares_the_three_entry_points():
    from gkgnet_amd import _abi, _lib
    protos = _abi.header().protos
    assert protos["gkg_linear_bf16_knn_prep_scratch_bytes"] == (Z, [I])
    assert protos["gkg_linear_bf16_knn_prep_supported"] == (I, [I] * 10 + [U, I])
    # x, ldx, wplanes, cin, a, cshift | the producers' shared run, as in gkg_affine_knn_prep | scratch, scratch_bytes, stream
    run = [F, I, I] + [I] * 9 + [U, I, I, F, F, P, Z]
    assert protos["gkg_linear_bf16_knn_prep"] == (I, [P, I, P, I, F, F] + run + [P, Z, P])
    assert protos["gkg_affine_knn_prep"][1][3:-1] == run                       # the same run, argument for argument
    for name in NAMES:
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION >= 15


def test_host_functions_answer_without_a_device():
    from gkgnet_amd import _abi, _lib
    lib = _lib.load()
    f = _lib.KNN_NORMALIZE
    sup = lib.gkg_linear_bf16_knn_prep_supported
    #   cin, B, G, c, N, M, k, d, has_y, has_relpos, flags, fused_mr
    assert sup(80, 2, 2, 40, 324, 324, 9, 1, 0, 1, f, 0) == 1
    assert sup(96, 2, 8, 12, 196, 196, 18, 2, 0, 0, f, 0) == 1                   # narrow groups, the 12-padding of cpad
    assert sup(80, 1, 2, 40, 1296, 324, 9, 1, 1, 1, f, 0) == 1                   # pooled keys
    assert sup(640, 2, 2, 320, 81, 81, 9, 3, 0, 0, f | _lib.KNN_FORCE_PREFILTER | _lib.KNN_RELPOS_UNIT, 0) == 1
    assert sup(24, 2, 4, 6, 324, 324, 9, 1, 0, 0, f, 0) == 0                     # c % 4 (G c = 24 passes the projection)
    assert sup(12, 2, 2, 40, 324, 324, 9, 1, 0, 0, f, 0) == 0                    # cin % 8
    assert sup(80, 2, 2, 40, 324, 324, 9, 1, 0, 1, f | _lib.KNN_BF16_CONTRACT, 0) == 0
    assert sup(80, 2, 2, 40, 16, 16, 9, 2, 0, 0, f, 0) == 0                      # k d > M: the k-NN plan refuses
    assert sup(80, 0, 2, 40, 324, 324, 9, 1, 0, 0, f, 0) == 0
    # one arrival counter per 128-row tile
    sb = lib.gkg_linear_bf16_knn_prep_scratch_bytes
    assert sb(0) == 0 and sb(1) == 4 and sb(128) == 4 and sb(129) == 8 and sb(648) == 24
    # argument checks come before anything touches a device
    assert lib.gkg_linear_bf16_knn_prep(None, 80, None, 80, None, None, None, 80, 0, 2, 2, 40, 324, 324, 9, 1, 0, 0, f, 0, 0, None,
                                        None, None, 0, None, 0, None) == _abi.header().constants["ERR_NULL"]


def test_switch_is_off_by_default():
    import os
    from gkgnet_amd import fused
    if "lin_bf16_prep" not in os.environ.get("GKG_ENABLE", ""):
        assert fused.LIN_BF16_PREP is False


def _objs(dtype=torch.bfloat16, training=False, groups=1):
    x = types.SimpleNamespace(dtype=dtype, shape=(648, 80))
    conv = types.SimpleNamespace(groups=groups, weight=types.SimpleNamespace(shape=(160, 80 // groups, 1, 1)))
    bn = types.SimpleNamespace(training=training, track_running_stats=True)
    return x, conv, bn


def _knn(**kw):
    from gkgnet_amd import _lib
    d = dict(B=2, G=2, c=80, N=324, M=324, k=9, d=1, has_y=0, has_rp=1, flags=_lib.KNN_NORMALIZE, fused_mr=0, as_keys=0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_dispatch_predicate_truth_table(monkeypatch):
    """One flipped input per row turns the dispatch off.  Plain Python objects: no CUDA tensor, no autocast context."""
    from gkgnet_amd import _lib, fused
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.bfloat16)
    sup = lambda R, cin, cout: (R, cin, cout) == (648, 80, 160)                  # noqa: E731
    psup = lambda cin, knn: cin == 80 and knn.c == 80                            # noqa: E731
    ok = fused.lin_bf16_prep_ok
    with torch.no_grad():
        lp = fused.lowp_inference()
    assert lp is True
    x, conv, bn = _objs()
    knn = _knn()
    ALL = "all"                                     # every supported shape; True applies the measured rule (its own test below)
    assert ok(ALL, lp, x, conv, bn, knn, supported=sup, prep_supported=psup) is True
    assert ok(ALL, lp, x, conv, bn, knn) is True                                 # the library's own answers (host code)
    assert ok(True, lp, x, conv, bn, knn, supported=sup, prep_supported=psup) is False        # 648 rows: outside the measured rule
    assert ok(False, lp, x, conv, bn, knn, supported=sup, prep_supported=psup) is False       # a switch off
    assert ok(ALL, lp, x, conv, bn, None, supported=sup, prep_supported=psup) is False       # no problem to prepare
    with torch.enable_grad():
        assert ok(ALL, fused.lowp_inference(), x, conv, bn, knn, supported=sup, prep_supported=psup) is False
    assert ok(ALL, lp, _objs(dtype=torch.float32)[0], conv, bn, knn, supported=sup, prep_supported=psup) is False
    assert ok(ALL, lp, x, conv, _objs(training=True)[2], knn, supported=sup, prep_supported=psup) is False
    assert ok(ALL, lp, x, _objs(groups=4)[1], bn, knn, supported=sup, prep_supported=psup) is False
    assert ok(ALL, lp, x, conv, bn, knn, chain=False, supported=sup, prep_supported=psup) is False
    assert ok(ALL, lp, x, conv, bn, knn, nchw=(2, 160, 18, 18), supported=sup, prep_supported=psup) is False
    for kw in ("scale", "xm"):
        assert ok(ALL, lp, x, conv, bn, knn, supported=sup, prep_supported=psup, **{kw: object()}) is False
    for kw in ("alias", "dual"):
        assert ok(ALL, lp, x, conv, bn, knn, supported=sup, prep_supported=psup, **{kw: True}) is False
    assert ok(ALL, lp, x, conv, bn, knn, supported=lambda *a: False, prep_supported=psup) is False
    assert ok(ALL, lp, x, conv, bn, knn, supported=sup, prep_supported=lambda *a: False) is False
    # a problem that is not this layer's output, or not a queries problem
    assert ok(ALL, lp, x, conv, bn, _knn(as_keys=1), supported=sup, prep_supported=psup) is False
    assert ok(ALL, lp, x, conv, bn, _knn(N=325), supported=sup, prep_supported=psup) is False
    assert ok(ALL, lp, x, conv, bn, _knn(G=4), supported=sup, prep_supported=psup) is False
    # the library says no: the bf16 contraction, k d > M
    assert ok(ALL, lp, x, conv, bn, _knn(flags=_lib.KNN_NORMALIZE | _lib.KNN_BF16_CONTRACT)) is False
    assert ok(ALL, lp, x, conv, bn, _knn(k=200, d=2)) is False
    # group widths that are no multiple of 4
    x2 = types.SimpleNamespace(dtype=torch.bfloat16, shape=(648, 80))
    conv2 = types.SimpleNamespace(groups=1, weight=types.SimpleNamespace(shape=(24, 80, 1, 1)))
    assert ok(ALL, lp, x2, conv2, bn, _knn(G=4, c=6)) is False



def test_measured_rule_takes_the_stage_one_shapes_only():
    """``on`` == True: the shapes where the one launch measured at least as fast as the two (linear_bf16.py: the table beside
    prep_pays) — GKGNet-576 and pvig_m at 768 x 768, stage 1, at their benchmark batch — and nothing narrower, wider or shorter."""
    from gkgnet_amd import _lib, fused, linear_bf16

    def case(B, N, C, G, M, k):
        x = types.SimpleNamespace(dtype=torch.bfloat16, shape=(B * N, C))
        conv = types.SimpleNamespace(groups=1, weight=types.SimpleNamespace(shape=(C, C, 1, 1)))
        bn = types.SimpleNamespace(training=False, track_running_stats=True)
        knn = _knn(B=B, G=G, c=C // G, N=N, M=M, k=k, has_y=int(M != N), flags=_lib.KNN_NORMALIZE | _lib.KNN_RELPOS_UNIT)
        return [fused.lin_bf16_prep_ok(on, True, x, conv, bn, knn) for on in (True, "all", False)]
    assert case(32, 144 * 144, 80, 2, 36 * 36, 9) == [True, True, False]            # cfg3 stage 1
    assert case(16, 192 * 192, 96, 8, 48 * 48, 18) == [True, True, False]           # cfg5 stage 1
    assert case(32, 72 * 72, 160, 2, 36 * 36, 9) == [False, True, False]            # cfg3 stage 2: two column tiles
    assert case(32, 18 * 18, 640, 2, 18 * 18, 9) == [False, True, False]            # cfg3 stage 4
    assert case(16, 96 * 96, 192, 8, 48 * 48, 18) == [False, True, False]           # cfg5 stage 2
    assert case(2, 144 * 144, 80, 2, 36 * 36, 9) == [False, True, False]            # stage 1 at a small batch: not measured
    assert linear_bf16.prep_pays(1 << 19, 128, 40) and not linear_bf16.prep_pays((1 << 19) - 1, 128, 40)
    assert not linear_bf16.prep_pays(1 << 20, 136, 40) and not linear_bf16.prep_pays(1 << 20, 96, 48)


def test_switch_values():
    """GKG_ENABLE=lin_bf16_prep applies the measured rule, lin_bf16_prep_all takes every supported shape (read at import)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for env, want in (("lin_bf16,lin_bf16_prep", "True True"), ("lin_bf16,lin_bf16_prep_all", "True all")):
        out = subprocess.run([sys.executable, "-c", "from gkgnet_amd import fused; print(fused.LIN_BF16, fused.LIN_BF16_PREP)"],
                             cwd=root, env=dict(os.environ, GKG_ENABLE=env), capture_output=True, text=True, check=True).stdout
        assert out.strip() == want, (env, out)


def test_lin_bf16_ok_still_refuses_a_layer_with_a_knn_problem(monkeypatch):
    from gkgnet_amd import fused
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.bfloat16)
    x, conv, bn = _objs()
    with torch.no_grad():
        lp = fused.lowp_inference()
    sup = lambda R, cin, cout: True                                              # noqa: E731
    assert fused.lin_bf16_ok(True, lp, x, conv, bn, supported=sup) is True
    assert fused.lin_bf16_ok(True, lp, x, conv, bn, knn=_knn(), supported=sup) is False
