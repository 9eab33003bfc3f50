"""The Python view of the C ABI is derived from include/gkg_hip.h (gkgnet_amd/_abi.py).  Host only: the parser on hand-written
snippets with the expected ctypes written out, its refusals, a handful of the real header's longest prototypes against literals
checked by hand, every struct's layout against the compiler's sizeof / offsetof, and the names the package reads."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gkgnet_amd import _abi  # noqa: E402

V, I, Z, F, U, LL = C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_uint, C.c_longlong


def test_the_parser_needs_neither_torch_nor_the_library():
    code = "import sys; from gkgnet_amd import _abi; _abi.header(); assert 'torch' not in sys.modules, 'torch imported'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ----------------------------------------------------------------------------------------------- snippets
SNIPPET = """
/* a block comment naming gkg_not_a_function(x) */
#ifndef GKG_SNIPPET_H_
#define GKG_SNIPPET_H_
#include <stddef.h>
#define GKG_ABI_VERSION 7
#define GKG_FLAG_A 4u   /* with a comment
                         * that runs on */
#define GKG_ERR_BAD -2
#define GKG_PROF_B 1
#define GKG_PROF_A 0
#define GKG_PROF_NUM 2
typedef struct GkgInner {
  const void* p; const float* q;   // line comment
  float momentum, eps;
  int cin, cout, nb;
  uint16_t* arg; int64_t* idx; long long* nbt;
  size_t n; unsigned flags; long long big;
} GkgInner;
typedef struct GkgOuter {
  int B;
  GkgInner fc1, conv, fc2;
  double* sums;
} GkgOuter;
int gkg_version(void);
const char* gkg_last_error_string(void);
void gkg_prof_reset(void);
unsigned long long gkg_capture_id(void* stream);
size_t gkg_bytes(int a, unsigned flags);
long long gkg_fill(void* host, long long unit_begin, long long* counter, double scale, long n);
double gkg_work(int id);
int gkg_block_bwd(const GkgOuter* b, GkgInner* wq /* [3] */,
                  const float* x, uint8_t* argmax,
                  float momentum, void* stream);
"""


def test_snippet_constants():
    k = _abi.parse(SNIPPET).constants
    assert k == {"ABI_VERSION": 7, "FLAG_A": 4, "ERR_BAD": -2, "PROF_B": 1, "PROF_A": 0, "PROF_NUM": 2}      # no include guard


def test_snippet_structs():
    s = _abi.parse(SNIPPET).structs
    assert list(s) == ["GkgInner", "GkgOuter"]
    inner, outer = s["GkgInner"], s["GkgOuter"]
    assert issubclass(inner, C.Structure) and issubclass(outer, C.Structure)
    assert inner._fields_ == [("p", V), ("q", V), ("momentum", F), ("eps", F), ("cin", I), ("cout", I), ("nb", I), ("arg", V),
                              ("idx", V), ("nbt", V), ("n", Z), ("flags", U), ("big", LL)]
    assert outer._fields_ == [("B", I), ("fc1", inner), ("conv", inner), ("fc2", inner), ("sums", V)]
    assert tuple(f[0] for f in outer._fields_ if f[1] is inner) == ("fc1", "conv", "fc2")


def test_snippet_prototypes():
    abi = _abi.parse(SNIPPET)
    inner, outer = abi.structs["GkgInner"], abi.structs["GkgOuter"]
    assert abi.protos == {
        "gkg_version": (I, []),
        "gkg_last_error_string": (C.c_char_p, []),
        "gkg_prof_reset": (None, []),
        "gkg_capture_id": (C.c_ulonglong, [V]),
        "gkg_bytes": (Z, [I, U]),
        "gkg_fill": (LL, [V, LL, V, C.c_double, C.c_long]),
        "gkg_work": (C.c_double, [I]),
        "gkg_block_bwd": (I, [C.POINTER(outer), C.POINTER(inner), V, V, F, V]),
    }
    assert list(abi.protos)[0] == "gkg_version" and list(abi.protos)[-1] == "gkg_block_bwd"          # declaration order


# ----------------------------------------------------------------------------------------------- loud failure
def _raises(text, *needles):
    with pytest.raises(_abi.GkgError) as e:
        _abi.parse(text)
    for n in needles:
        assert n in str(e.value), (n, str(e.value))


def test_unknown_types_are_named_not_guessed():
    _raises("int gkg_f(hipStream_t stream);", "hipStream_t stream")
    _raises("int gkg_f(int a, uint16_t half);", "uint16_t half")
    _raises("int gkg_f(int);", "'int'")                                            # an unnamed parameter
    _raises("bool gkg_f(int a);", "bool")
    _raises("typedef struct GkgS { int a; short b; } GkgS;", "short b")
    _raises("typedef struct GkgS { int a[4]; } GkgS;", "int a[4]")
    _raises("#define GKG_X (1 << 3)", "GKG_X (1 << 3)")
    _raises("struct GkgS { int a; };", "struct GkgS")


def test_a_pointer_declaration_with_several_declarators_is_rejected():
    _raises("typedef struct GkgS { float* a, b; } GkgS;", "float* a, b")
    _raises("typedef struct GkgS { float *a, *b; } GkgS;", "float *a, *b")


def test_a_named_entry_point_that_does_not_parse_fails_the_count():
    ok = "int gkg_a(int x);\n"
    assert list(_abi.parse(ok).protos) == ["gkg_a"]
    _raises(ok + "int gkg_foo(int (*callback)(int), void* stream);", "gkg_foo", "2 entry points named, 1 prototypes bound")
    _raises(ok + "int gkg_foo(int x)\n", "gkg_foo")                                 # no terminating semicolon


def test_a_missing_header_says_where_it_was_looked_for(monkeypatch, tmp_path):
    missing = str(tmp_path / "include" / "gkg_hip.h")
    monkeypatch.setattr(_abi, "HEADER", missing)
    with pytest.raises(_abi.GkgError) as e:
        _abi.header.__wrapped__()                        # (past the cache: the process's one parse stays the one everybody holds)
    assert missing in str(e.value)


def test_the_header_is_parsed_once_per_process():
    assert _abi.header() is _abi.header()
    assert _abi.HEADER == os.path.join(ROOT, "include", "gkg_hip.h")


# ----------------------------------------------------------------------------------------------- the real header
def test_long_prototypes_against_hand_checked_literals():
    """Each list below was written from the prototype in include/gkg_hip.h, one row per line of the declaration, and checked by
    hand: the signatures where a count slip was most likely when the table was kept as `[V] * 13 + [I] * 11 + ...`."""
    abi = _abi.header()
    S = abi.structs
    want = {
        "gkg_bn_eval_bwd": (I, [V, V, V, V, V, I, I, I,                   # dout y a c dy R C nb
                                I, Z, I, V, I,                            # ldg dout_bstride act row_scale rows_per_scale
                                V, V, V, F, V,                            # running_mean running_var bias eps dgamma
                                V, V, V, V, Z, V,                         # dbeta dbias sums zero_buf zero_doubles workspace
                                Z, V]),                                   # workspace_bytes stream
        "gkg_bn_apply_knn_prep": (I, [V, V, V, V, V,                      # y sums gamma beta bias
                                      V, V, V, V, V,                      # running_mean running_var num_batches_tracked a c_out
                                      V, V, V, I, I, I, I, I, I, I, I,    # mean invstd out ldo ochunk B G c N M k
                                      I, I, I, U, I, I, V,                # dilation has_y has_relpos knn_flags fused_mr as_keys res_tm
                                      V, V, Z, F, F, V,                   # out_nchw knn_workspace knn_workspace_bytes momentum eps zero_buf
                                      Z, V]),                             # zero_doubles stream
        "gkg_linear_dgrad_x6_sk": (I, [V, I, Z, V, V, I, I,               # dy ldg g_bstride planes_dgrad dx R cin
                                       I, I, V, V, Z, I,                  # cout nb residual splitk_ws splitk_bytes ldx
                                       Z, U, V]),                         # x_bstride flags stream
        "gkg_knn_fwd_tm": (I, [V, I, I, V, V, V, V,                       # x ldx xchunk y relpos nn_idx center
                               I, I, I, I, I, I, I, I, U,                 # B G c N M k dilation dtype flags
                               V, Z, V]),                                 # workspace workspace_bytes stream
        "gkg_x6_prep_desc_fill": (LL, [V, I, V, V, V, I,                  # host_descs index w planes_fwd planes_dgrad cin
                                       I, I, LL, I]),                     # cout nb unit_begin kperm
        "gkg_linear_wgrad_x6_batch": (I, [C.POINTER(S["GkgWgradProblem"]), I, I, V]),
        "gkg_grapher_bwd": (I, [C.POINTER(S["GkgGrapherBlock"]), C.POINTER(S["GkgWgradProblem"]), V]),
        "gkg_grapher_label_fwd": (I, [C.POINTER(S["GkgLabelBlock"]), V]),
        "gkg_prof_read": (I, [I, V, V]),
        "gkg_last_error_string": (C.c_char_p, []),
        "gkg_prof_reset": (None, []),
        "gkg_stream_capture_id": (C.c_ulonglong, [V]),
    }
    assert len(want["gkg_bn_eval_bwd"][1]) == 26 and len(want["gkg_bn_apply_knn_prep"][1]) == 36
    for name, sig in want.items():
        assert abi.protos[name] == sig, name


def _hipcc():
    from gkgnet_amd import _build
    cc = _build._hipcc()
    return cc if (os.path.exists(cc) or shutil.which(cc)) else None


def test_struct_layout_matches_the_compilers(tmp_path):
    """sizeof of every struct and offsetof of every field, printed by a program generated from the parsed field names and compiled
    host-only against include/gkg_hip.h, equal ctypes' — one line per number."""
    if _hipcc() is None:
        pytest.skip("no hipcc")
    structs = _abi.header().structs
    want, body = [], []
    for sname, cls in structs.items():
        want.append("%s %d" % (sname, C.sizeof(cls)))
        body.append('  printf("%s %%zu\\n", sizeof(%s));' % (sname, sname))
        for fname, _ in cls._fields_:
            want.append("%s.%s %d" % (sname, fname, getattr(cls, fname).offset))
            body.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (sname, fname, sname, fname))
    src, exe = tmp_path / "abi_layout.cpp", tmp_path / "abi_layout"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "gkg_hip.h"\nint main() {\n%s\n  return 0;\n}\n' % "\n".join(body))
    subprocess.check_call([_hipcc(), "--cuda-host-only", "-x", "hip", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    got = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    assert got == want
    assert len(want) == len(structs) + sum(len(c._fields_) for c in structs.values()) and len(structs) == 5
    assert [C.sizeof(c) for c in structs.values()] == [int(ln.split()[1]) for ln in got if "." not in ln]


# ----------------------------------------------------------------------------------------------- the names the package reads
def test_every_name_read_through_lib_resolves_with_the_headers_value():
    from gkgnet_amd import _lib
    k = _abi.header().constants
    used = set()
    for top in ("gkgnet_amd", "tools", "tests"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(".py"):
                    with open(os.path.join(dirpath, f)) as fh:
                        used |= set(re.findall(r"\b_lib\.([A-Za-z_]\w*)", fh.read()))
    assert {"F32", "KNN_NORMALIZE", "WgradProblem", "GkgError", "load", "check"} <= used
    missing = sorted(n for n in used if not hasattr(_lib, n))
    assert not missing, missing
    consts = {n for n in used if n.isupper() and isinstance(getattr(_lib, n), int)}
    assert consts <= set(k), sorted(consts - set(k))                               # every flag / code read is one the header defines
    for n in set(k) & set(vars(_lib)):
        assert getattr(_lib, n) == k[n], n
    assert _lib.ABI_VERSION == k["ABI_VERSION"] and _lib.ERR_UNSUPPORTED == k["ERR_UNSUPPORTED"] == -3
    assert _lib.PROF_KERNELS == ("token_prep", "knn_tile", "knn_merge", "mr_fwd", "mr_bwd", "gemm_x6")
    assert len(_lib.PROF_KERNELS) == k["PROF_NUM"]
    assert _lib.EXPORTS == tuple(_abi.header().protos) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert _lib.WgradProblem is _abi.header().structs["GkgWgradProblem"]
    assert _lib.GkgError is _abi.GkgError


def test_block_descriptors_are_the_derived_classes():
    from gkgnet_amd import block
    s = _abi.header().structs
    assert (block.ProjBN, block.GraphOp, block.GrapherBlock, block.LabelBlock) == (s["GkgProjBN"], s["GkgGraphOp"],
                                                                                   s["GkgGrapherBlock"], s["GkgLabelBlock"])
    names = lambda cls: tuple(f[0] for f in cls._fields_ if f[1] is block.ProjBN)          # noqa: E731  (block._finish_plan's rule)
    assert names(block.GrapherBlock) == ("fc1", "conv", "fc2")
    assert names(block.LabelBlock) == ("fc1", "conv", "fc2", "ffn1", "ffn2")
