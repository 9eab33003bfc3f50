#!/usr/bin/env python3
"""Record the bits of the deterministic x6 weight gradients (gkg_linear_wgrad_x6_det / _batch_det) as fixtures for
tests/test_hip_wgrad_split_bits.py.

Run it on the build whose bits are to be kept — the commit BEFORE a change to the weight-gradient loop — never on the code under
test:

    python tools/gen_wgrad_split_golden.py [--out tests/golden]

The det entry points are run-independent by construction, so one recording is the definition of "every dW partial keeps its
bits".  The cases, their operands (numpy RandomState: the same values on every machine) and the calls live here; the test imports
them from this file, so generator and test cannot drift apart.

Shapes (R, cout, cin, nb, kperm, slabs): the smallest that reach every path of the two LDS-DMA bodies.  A slab of 2 units of 128
rows is T = 4 steps per wave (prologue + ONE loop trip + the two peeled steps), of 4 units T = 8, of 3 units T = 6.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SINGLE_FILE, BATCH_FILE = "wgrad_split_single.npz", "wgrad_split_batch.npz"

# name -> (R, cout, cin, nb, kperm, slabs, operands); stand-alone plan (x6_wgrad_plan, batched = 0)
SINGLE = {
    "wide_interior_t4": (256, 64, 128, 1, 0, 1, "normal"),       # 64 x 128 body, no edge tile
    "wide_swap_edges_t8": (512, 80, 160, 1, 0, 1, "normal"),     # roles exchanged (transposed store), partial blocks on both sides
    "wide_edges_t4": (256, 80, 96, 1, 0, 1, "normal"),           # 64 x 128 body, roles as given, partial blocks on both sides
    "wide_edges_t6_two_slabs": (768, 80, 96, 1, 0, 2, "normal"),
    "dma_groups_kperm_t4": (256, 160, 160, 4, 1, 1, "normal"),   # 64 x 64 body, 3 x 3 tiles with edges, four groups, [x | m] columns
    "dma_one_edge_tile_t8": (512, 48, 40, 1, 0, 1, "normal"),
    "dma_interior_t8": (512, 64, 192, 1, 0, 1, "normal"),        # 64 x 64 body, no edge tile
    "wide_special_t8": (512, 80, 96, 1, 0, 1, "special"),
    "dma_special_t4": (256, 48, 40, 1, 0, 1, "special_swapped"),
}
# name -> (units_per_slab, [(R, cout, cin, nb, kperm, operands), ...]); batched plan (body "by matrix cost")
BATCH = {
    "ups2": (2, [(512, 160, 160, 4, 1, "normal"),                # wide body, 3 x 2 tiles with edges, two slabs shared by 4 XCDs each
                 (256, 64, 128, 1, 0, "normal"),
                 (512, 48, 40, 1, 0, "normal"),                  # 64 x 64 body, one edge tile
                 (256, 80, 160, 1, 0, "normal")]),               # wide body, roles exchanged
    "ups4": (4, [(512, 80, 96, 1, 0, "normal"),
                 (512, 64, 64, 1, 0, "normal"),                  # 64 x 64 body, interior
                 (512, 48, 40, 1, 0, "special_swapped"),
                 (512, 80, 160, 1, 0, "special")]),
}
# of a four-group result only these groups are recorded (every group runs the same code at another batch offset)
GROUPS_KEPT = (0, 3)


def _bf16_exact(a):
    return (a.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _special(rng, shape, big):
    """Exact bf16 values, +-0, magnitudes 1e-40 .. 1e-30 (denormal operands and denormal residuals) and full-precision normals; `big`:
    one element in 64 is of magnitude 1e30 .. 1e38 (finite after bf16 rounding).  The OTHER operand of the case is built with
    big = False and everything of order one scaled by 2^-12, so that no sum of products overflows: the recorded bits hold no NaN."""
    scale = np.float32(1.0 if big else 2.0 ** -12)
    n = int(np.prod(shape))
    cls = rng.randint(0, 64, n)
    sign = np.where(rng.randint(0, 2, n) == 0, np.float32(1), np.float32(-1)).astype(np.float32)
    normal = rng.standard_normal(n).astype(np.float32) * scale
    tiny = (10.0 ** rng.uniform(-40, -30, n)).astype(np.float32) * sign
    huge = (10.0 ** rng.uniform(30, 38, n)).astype(np.float32) * sign
    out = normal.copy()
    out = np.where(cls < 16, _bf16_exact(normal), out)
    out = np.where((cls >= 16) & (cls < 24), np.float32(0) * sign, out)
    out = np.where((cls >= 24) & (cls < 40), tiny, out)
    if big:
        out = np.where(cls == 63, huge, out)
    return out.astype(np.float32).reshape(shape)


def operands(R, cout, cin, nb, kind, seed):
    """(dy (nb, R, cout), x (nb, R, cin)) as contiguous float32 numpy arrays."""
    rng = np.random.RandomState(seed)
    if kind == "normal":
        return (rng.standard_normal((nb, R, cout)).astype(np.float32), (2 * rng.standard_normal((nb, R, cin))).astype(np.float32))
    if kind == "special":
        return _special(rng, (nb, R, cout), True), _special(rng, (nb, R, cin), False)
    if kind == "special_swapped":
        return _special(rng, (nb, R, cout), False), _special(rng, (nb, R, cin), True)
    raise ValueError(kind)


def _seed(name, i=0):
    return (sum(ord(c) * (k + 1) for k, c in enumerate(name)) + 7919 * i) % (2 ** 31)


def run_single(name):
    """dw (nb, cout, cin) of case `name` as a cuda float32 tensor."""
    import torch
    from gkgnet_amd import _lib as L
    lib = L.load()
    R, cout, cin, nb, kperm, slabs, kind = SINGLE[name]
    dy, x = (torch.from_numpy(a).cuda() for a in operands(R, cout, cin, nb, kind, _seed(name)))
    n = lib.gkg_linear_wgrad_x6_det_workspace_bytes(R, cin, cout, nb, cout, cin, slabs)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    dw = torch.full((nb, cout, cin), 7.0, device="cuda")
    L.check(lib.gkg_linear_wgrad_x6_det(dy.data_ptr(), cout, R * cout, x.data_ptr(), cin, R * cin, dw.data_ptr(), R, cin, cout, nb,
                                        kperm, slabs, ws.data_ptr(), n, None), "gkg_linear_wgrad_x6_det")
    torch.cuda.synchronize()
    return dw


def run_batch(name):
    """[dw of every problem of batch `name`]"""
    import torch
    from gkgnet_amd import _lib as L
    lib = L.load()
    ups, probs = BATCH[name]
    keep, dws, arr = [], [], []
    for i, (R, cout, cin, nb, kperm, kind) in enumerate(probs):
        dy, x = (torch.from_numpy(a).cuda() for a in operands(R, cout, cin, nb, kind, _seed(name, i + 1)))
        dw = torch.full((nb, cout, cin), 7.0, device="cuda")
        keep += [dy, x]
        dws.append(dw)
        arr.append(L.WgradProblem(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), R * cout, R * cin, cout, cin, R, cin, cout, nb, kperm))
    arr = (L.WgradProblem * len(arr))(*arr)
    n = lib.gkg_linear_wgrad_x6_batch_det_workspace_bytes(arr, len(probs), ups)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    L.check(lib.gkg_linear_wgrad_x6_batch_det(arr, len(probs), ups, ws.data_ptr(), n, None), "gkg_linear_wgrad_x6_batch_det")
    torch.cuda.synchronize()
    return dws


def recorded(dw):
    """What of a result is kept in the fixture: its bits as uint32, of a four-group result the groups GROUPS_KEPT."""
    a = dw.detach().cpu().numpy().view(np.uint32)
    return a[list(GROUPS_KEPT)] if a.shape[0] == 4 else a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    single = {k: recorded(run_single(k)) for k in SINGLE}
    batch = {}
    for k in BATCH:
        for i, dw in enumerate(run_batch(k)):
            batch[f"{k}_{i}"] = recorded(dw)
    for d in (single, batch):
        for k, a in d.items():
            f = a.view(np.float32)
            assert np.isfinite(f).all(), k                     # no NaN payloads, no infinities in the record
            assert np.count_nonzero(f) > f.size // 2, k
    np.savez(os.path.join(args.out, SINGLE_FILE), **single)
    np.savez(os.path.join(args.out, BATCH_FILE), **batch)
    for fn in (SINGLE_FILE, BATCH_FILE):
        print(fn, os.path.getsize(os.path.join(args.out, fn)), "bytes")


if __name__ == "__main__":
    main()
