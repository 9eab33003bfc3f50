"""ctypes binding of libgkg_hip.so (C ABI: include/gkg_hip.h).

The product has NO CPU fallback: if the library is missing or a call fails this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _abi
from ._abi import GkgError  # noqa: F401  (the package's error type; raised from here on)

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GKG_HIP_LIB") or os.path.join(PKG, "libgkg_hip.so")   # GKG_HIP_LIB: same-box A/B of two builds (tools)

# The names the package uses, with include/gkg_hip.h's values (_abi.py reads the header): no value, field list or argument list
# of the ABI is restated in Python.
_ABI = _abi.header()
_K = _ABI.constants
ABI_VERSION = _K["ABI_VERSION"]
F32, BF16, F16 = _K["F32"], _K["BF16"], _K["F16"]
KNN_NORMALIZE = _K["KNN_NORMALIZE"]
KNN_BF16_CONTRACT = _K["KNN_BF16_CONTRACT"]
KNN_SELECT_DIRECT = _K["KNN_SELECT_DIRECT"]
KNN_SELECT_BUFFERED = _K["KNN_SELECT_BUFFERED"]
KNN_NO_PREFILTER = _K["KNN_NO_PREFILTER"]
KNN_FORCE_PREFILTER = _K["KNN_FORCE_PREFILTER"]
KNN_RELPOS_UNIT = _K["KNN_RELPOS_UNIT"]
KNN_X_PREPARED = _K["KNN_X_PREPARED"]
KNN_Y_PREPARED = _K["KNN_Y_PREPARED"]
KNN_F16_CONTRACT = _K["KNN_F16_CONTRACT"]
MR_DETERMINISTIC, MR_FP32_ATOMICS = _K["MR_DETERMINISTIC"], _K["MR_FP32_ATOMICS"]
X6_NO_KS, X6_FORCE_KS = _K["X6_NO_KS"], _K["X6_FORCE_KS"]
X6_NO_WALK, X6_FORCE_WALK, X6_WALK_CAP_SHIFT = _K["X6_NO_WALK"], _K["X6_FORCE_WALK"], _K["X6_WALK_CAP_SHIFT"]
ERR_UNSUPPORTED = _K["ERR_UNSUPPORTED"]
BLOCK_NO_BWD_FUSE, BLOCK_NO_DGRAD_STATS, BLOCK_NO_X6_WALK = _K["BLOCK_NO_BWD_FUSE"], _K["BLOCK_NO_DGRAD_STATS"], _K["BLOCK_NO_X6_WALK"]
EXPORTS = tuple(_ABI.protos)
# the profiler's kernel ids GKG_PROF_* (all but the count GKG_PROF_NUM) as lower-case names, in id order
PROF_KERNELS = tuple(n[5:].lower() for n in sorted((n for n in _K if n.startswith("PROF_") and n != "PROF_NUM"), key=_K.get))
WgradProblem = _ABI.structs["GkgWgradProblem"]

_RELPOS_WARNED = False


def relpos_flags(rp) -> int:
    """KNN_RELPOS_UNIT when every |relative_pos| <= 1.125 (the prefilter kernel's precondition, include/gkg_hip.h).  The check
    is one reduction + a host read, cached ON the tensor object (keyed on its version counter): a module's frozen
    ``relative_pos`` parameter pays it once, in the eager warm-up; a tensor first seen inside a hipGraph capture is not
    vouched for (the call then takes the fp32 tile kernel: same results)."""
    if rp is None:
        return 0
    import torch
    ent = getattr(rp, "_gkg_unit", None)
    if ent is None or ent[0] != rp._version:
        if torch.cuda.is_current_stream_capturing():
            # the range check needs a host read, which a capture cannot make: this call takes the fp32 tile kernel (same graphs,
            # slower for long key streams).  Said once — a user who captures on step 0 loses the prefilter otherwise unnoticed.
            global _RELPOS_WARNED
            if not _RELPOS_WARNED:
                _RELPOS_WARNED = True
                import warnings
                warnings.warn("gkgnet_amd: a relative_pos tensor was first seen inside a hipGraph capture; its value range cannot be "
                              "checked there, so the k-NN of this capture runs without the bf16 prefilter (identical graphs, slower "
                              "at long key streams).  Run one eager warm-up forward before capturing.", RuntimeWarning, stacklevel=3)
            return 0
        ent = (rp._version, bool((rp.detach().abs().max() <= 1.125).item()))
        try:
            rp._gkg_unit = ent
        except AttributeError:
            pass
    return KNN_RELPOS_UNIT if ent[1] else 0


def knn_select_flags() -> int:
    """GKG_KNN_SELECT=direct|buffered, GKG_KNN_PREFILTER=0|force (measurement / tests) -> the C API's mode flags; read here,
    per call, so the library's launch path never calls getenv."""
    sel = os.environ.get("GKG_KNN_SELECT", "")
    f = KNN_SELECT_BUFFERED if sel[:1] == "b" else (KNN_SELECT_DIRECT if sel[:1] == "d" else 0)
    pf = os.environ.get("GKG_KNN_PREFILTER", "")
    if pf == "0" or f:                                             # a forced selection mode means the fp32 tile kernel
        f |= KNN_NO_PREFILTER
    elif pf == "force":
        f |= KNN_FORCE_PREFILTER
    return f


_lib = None


def load():
    """Loads the HIP library (once).  Raises GkgError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch must own the process's HIP runtime: import it BEFORE dlopen-ing our library so that our
    # DT_NEEDED libamdhip64 resolves to the runtime torch already loaded (two runtimes in one process
    # -> "no ROCm-capable device" on the second one).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise GkgError(f"{LIB_PATH} not found: build it with `python -m gkgnet_amd._build` "
                       "(or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    _abi.bind(lib)
    v = lib.gkg_version()
    if v != ABI_VERSION:
        raise GkgError(f"libgkg_hip.so ABI {v} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().gkg_last_error_string().decode(errors="replace")
        raise GkgError(f"{what} failed (rc={rc}): {msg}")


def prof_enable(on: bool = True):
    load().gkg_prof_enable(1 if on else 0)


def prof_reset():
    load().gkg_prof_reset()


def prof_work(name):
    """Algorithmic flop of the launches counted for ``name`` since the last reset (kernels that report it)."""
    return load().gkg_prof_work(PROF_KERNELS.index(name))


def prof_read():
    """{kernel name: (total_ms, launches)} measured with HIP events on the launch stream."""
    lib = load()
    out = {}
    for i, name in enumerate(PROF_KERNELS):
        ms, cnt = C.c_double(0), C.c_long(0)
        check(lib.gkg_prof_read(i, C.byref(ms), C.byref(cnt)), "gkg_prof_read")
        out[name] = (ms.value, cnt.value)
    return out
