"""GKG_ENABLE=knn_f16 (GKG_KNN_F16_CONTRACT), the parts that need no device: the flag's value, the flag word of a k-NN problem, the
switch's parsing and default, which contraction a call takes when both 16-bit switches are on, and the library's host-side answers."""
import os
import re
import subprocess
import sys

import pytest
import torch

from gkgnet_amd import _lib, knn_prep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_is_the_headers_next_free_bit():
    text = open(os.path.join(ROOT, "include", "gkg_hip.h")).read()
    m = re.search(r"#define GKG_KNN_F16_CONTRACT (\d+)u", text)
    assert m and int(m.group(1)) == _lib._K["KNN_F16_CONTRACT"] == _lib.KNN_F16_CONTRACT
    assert _lib.KNN_F16_CONTRACT == 2 * _lib.KNN_Y_PREPARED
    others = [v for n, v in _lib._K.items() if n.startswith("KNN_") and n != "KNN_F16_CONTRACT"]
    assert all(v & _lib.KNN_F16_CONTRACT == 0 for v in others)


def test_problem_flags_sets_the_bit(monkeypatch):
    monkeypatch.setattr(_lib, "relpos_flags", lambda t: 0 if t is None else _lib.KNN_RELPOS_UNIT)
    for t in (None, torch.zeros(1, 4, 4)):
        base = knn_prep.problem_flags(t)
        assert base & (_lib.KNN_F16_CONTRACT | _lib.KNN_BF16_CONTRACT) == 0
        assert knn_prep.problem_flags(t, f16_contract=True) == base | _lib.KNN_F16_CONTRACT
        assert knn_prep.problem_flags(t, False, True) == base | _lib.KNN_F16_CONTRACT
        assert knn_prep.problem_flags(t, True, True) == base | _lib.KNN_BF16_CONTRACT          # never both bits: bf16 wins


def test_the_fp16_contraction_never_reads_prepared_queries():
    class Lib:
        def gkg_knn_workspace_bytes(self, *a):
            return 4096
    flags = knn_prep.problem_flags(None, f16_contract=True)
    p = knn_prep.KnnProblem(3, 2, 32, 20, 144, 9, 1, 1, None, 0, flags)
    x = torch.zeros(4)
    p.producer_args(Lib(), x, None, None, 8, 2)
    p.mark(x)
    ws, got = knn_prep.consumer_ws_flags(Lib(), x, 3, 2, 32, 20, 144, 9, 1, 1, 0, flags, 0)
    assert got == flags and ws is not p.ws


@pytest.mark.parametrize("env,want", [("", "False False"), ("knn_f16", "False True"), ("knn_bf16", "True False"),
                                      ("lin_bf16, knn_f16 ,knn_bf16", "True True")])
def test_gkg_enable_parsing(env, want):
    out = subprocess.run([sys.executable, "-c", "from gkgnet_amd import fused; print(fused.KNN_BF16, fused.KNN_F16)"], cwd=ROOT,
                         env=dict(os.environ, GKG_ENABLE=env), capture_output=True, text=True, check=True).stdout
    assert out.split() == want.split()


def test_switch_is_off_by_default_and_documented():
    from gkgnet_amd import fused
    if "knn_f16" not in os.environ.get("GKG_ENABLE", ""):
        assert fused.KNN_F16 is False
    assert "knn_f16" in open(fused.__file__).read().split("_DISABLED = _env_list")[0]      # the GKG_ENABLE comment table


@pytest.mark.parametrize("bf,hf,dtype,want", [
    (False, False, torch.bfloat16, None), (True, False, torch.bfloat16, "bf16"), (False, True, torch.bfloat16, "f16"),
    (True, True, torch.bfloat16, "bf16"),                                          # both on: bf16 wins
    (False, True, torch.float16, "f16"), (True, False, torch.float16, None), (True, True, torch.float16, "f16"),
    (True, True, torch.float32, None), (True, True, None, None)])                  # dtype None: autocast off
def test_which_contraction_a_call_takes(monkeypatch, bf, hf, dtype, want):
    from gkgnet_amd import block, fused
    monkeypatch.setattr(fused, "KNN_BF16", bf)
    monkeypatch.setattr(fused, "KNN_F16", hf)
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: dtype is not None)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda dev: dtype)
    assert fused.knn_contract() == want
    # tokens are prepared ahead (fused k-NN + aggregation, prepared queries, lin_bf16_prep) only without a 16-bit contraction switch
    assert fused._knn_ahead_ok() == (not ((bf or hf) and dtype is not None))
    keys = set()
    for v in (False, True):                                                        # the block driver's cache key sees the switch
        monkeypatch.setattr(fused, "KNN_F16", v)
        keys.add(block._switches())
    assert len(keys) == 2


def test_host_functions_answer_zero_with_the_flag():
    lib = _lib.load()
    f = _lib.KNN_NORMALIZE
    assert lib.gkg_knn_mr_fused_supported(32, 4, 80, 324, 324, 9, 1, 0, 1, f) == 1
    assert lib.gkg_knn_mr_fused_supported(32, 4, 80, 324, 324, 9, 1, 0, 1, f | _lib.KNN_F16_CONTRACT) == 0
    assert lib.gkg_linear_bf16_knn_prep_supported(80, 2, 2, 40, 324, 324, 9, 1, 0, 1, f, 0) == 1
    assert lib.gkg_linear_bf16_knn_prep_supported(80, 2, 2, 40, 324, 324, 9, 1, 0, 1, f | _lib.KNN_F16_CONTRACT, 0) == 0
    # the workspace plan is the bf16 form's (and the exact form's: one plan)
    q = lib.gkg_knn_workspace_bytes
    assert q(4, 40, 324, 324, 9, 1, _lib.F32, f | _lib.KNN_F16_CONTRACT) == q(4, 40, 324, 324, 9, 1, _lib.F32, f | _lib.KNN_BF16_CONTRACT) > 0
