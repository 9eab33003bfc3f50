"""Every dW partial of the LDS-DMA weight-gradient bodies keeps its bits: gkg_linear_wgrad_x6_det and _batch_det (run-independent by
construction) against arrays recorded from the library of the commit before the loop's instruction stream was changed
(tests/golden/wgrad_split_*.npz, written by tools/gen_wgrad_split_golden.py, which also owns the cases and their operands).

The shapes are the smallest that reach every path: slabs of 2, 3 and 4 units of 128 rows (one loop trip after the prologue, and
more), the 64 x 64 and the 64 x 128 body each with and without edge tiles, exchanged operand roles, four groups with the [x | m]
column permutation, and operands that mix exact bf16 values, signed zeros, denormals and magnitudes up to 1e38."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_wgrad_split_golden", os.path.join(ROOT, "tools", "gen_wgrad_split_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name))


def _same_bits(got, want, what):
    got = G.recorded(got)
    assert got.shape == want.shape and want.dtype == np.uint32, what
    differ = int((got != want).sum())
    if differ:
        i = tuple(int(v[0]) for v in np.nonzero(got != want))
        print(f"{what}: {differ} of {want.size} elements differ, first at {i}: got {got[i]:#010x} ({got.view(np.float32)[i]!r}), "
              f"recorded {want[i]:#010x} ({want.view(np.float32)[i]!r})")
    assert differ == 0, what


def test_the_fixtures_cover_the_cases():
    assert sorted(_golden(G.SINGLE_FILE).files) == sorted(G.SINGLE)
    assert sorted(_golden(G.BATCH_FILE).files) == sorted(f"{k}_{i}" for k, (_, probs) in G.BATCH.items() for i in range(len(probs)))


@pytest.mark.parametrize("name", sorted(G.SINGLE))
def test_wgrad_x6_det_keeps_the_recorded_bits(name):
    _same_bits(G.run_single(name), _golden(G.SINGLE_FILE)[name], name)


@pytest.mark.parametrize("name", sorted(G.BATCH))
def test_wgrad_x6_batch_det_keeps_the_recorded_bits(name):
    gold = _golden(G.BATCH_FILE)
    for i, dw in enumerate(G.run_batch(name)):
        _same_bits(dw, gold[f"{name}_{i}"], f"{name}, problem {i}")
