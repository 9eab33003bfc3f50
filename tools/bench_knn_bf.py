#!/usr/bin/env python
"""k-NN kernel time under a 16-bit contraction flag (the cfg3 / cfg5 inference forms) per stage shape, with and without
relative_pos — library-side HIP-event timing.    python tools/bench_knn_bf.py [--format bf16|f16|alt] [shape ...]
--format alt: per shape bf16, f16 and bf16 once more on the same inputs in one process (the second bf16 run is the run-to-run
spread the f16 figure is read against)."""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gkgnet_amd import _lib

SHAPES = {   # name: (BG, c, N, M(None=self), k, d, relpos)
    "s1": (64, 40, 20736, 1296, 9, 1, True), "s1_norp": (64, 40, 20736, 1296, 9, 1, False),
    "s2": (64, 80, 5184, 1296, 9, 1, True), "s2_norp": (64, 80, 5184, 1296, 9, 1, False),
    "s3_d2": (64, 200, 1296, None, 9, 2, True), "s3_d3": (64, 200, 1296, None, 9, 3, True),
    "m1": (128, 12, 36864, 2304, 18, 1, True), "m1_norp": (128, 12, 36864, 2304, 18, 1, False),
    "m2": (128, 24, 9216, 2304, 18, 1, True), "m3_d2": (128, 48, 2304, None, 18, 2, True),
    "m3_d2_norp": (128, 48, 2304, None, 18, 2, False), "m4_d2": (128, 96, 576, None, 18, 2, True),
}
FORMATS = {"bf16": "KNN_BF16_CONTRACT", "f16": "KNN_F16_CONTRACT"}


def run(name, formats=("bf16",), iters=5):
    BG, c, N, M, k, d, has_rp = SHAPES[name]
    lib = _lib.load()
    torch.manual_seed(0)
    x = torch.randn(BG, c, N, device="cuda")
    y = None if M is None else torch.randn(BG, c, M, device="cuda")
    Mk = N if M is None else M
    rp = -torch.rand(N, Mk, device="cuda") if has_rp else None
    edge = torch.empty((1, BG, N, k), dtype=torch.int64, device="cuda")
    for fmt in formats:
        flags = _lib.KNN_NORMALIZE | getattr(_lib, FORMATS[fmt]) | _lib.knn_select_flags()
        ws = torch.empty(int(lib.gkg_knn_workspace_bytes(BG, c, N, Mk, k, d, _lib.F32, flags)), dtype=torch.uint8, device="cuda")

        def call():
            _lib.check(lib.gkg_knn_fwd(x.data_ptr(), None if y is None else y.data_ptr(), None if rp is None else rp.data_ptr(),
                                       edge.data_ptr(), None, BG, c, N, Mk, k, d, _lib.F32, flags, ws.data_ptr(), ws.numel(), None),
                       "gkg_knn_fwd")
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        _lib.prof_reset(); _lib.prof_enable(True)
        for _ in range(iters):
            call()
        torch.cuda.synchronize()
        _lib.prof_enable(False)
        out = {"shape": name, "format": fmt}
        for kn, (ms, cnt) in _lib.prof_read().items():
            if cnt:
                out[kn + "_us"] = round(1e3 * ms / iters, 1)
        rp_gb = (4.0 * N * Mk * BG / 1e9) if has_rp else 0.0
        out["relpos_reads_GB"] = round(rp_gb, 2)
        if has_rp and "knn_tile_us" in out:
            out["relpos_TBs"] = round(rp_gb / out["knn_tile_us"] * 1e3, 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    fmt = "bf16"
    if "--format" in args:
        i = args.index("--format")
        fmt = args[i + 1]
        del args[i:i + 2]
    if fmt not in ("bf16", "f16", "alt"):
        sys.exit(f"--format {fmt}: expected bf16 | f16 | alt")
    for n in (args or list(SHAPES)):
        run(n, ("bf16", "f16", "bf16") if fmt == "alt" else (fmt,))
