"""The Python view of the C ABI, read from include/gkg_hip.h.

Every .hip file includes that header, so the compiler checks the C definitions against it; this module is what checks the Python
side: constants, descriptor structs and prototypes become ctypes objects by rule, and a declaration the rules do not cover raises
GkgError naming its text — nothing is guessed.  Pure Python (no torch, no library): ``parse`` takes any header text.

  #define GKG_<NAME> <integer>[u]        -> constants["<NAME>"]          (a define without a value — the include guard — is skipped)
  typedef struct X { ... } X;            -> structs["X"], a ctypes.Structure: pointer fields c_void_p, earlier structs by value
  <ret> gkg_name(<parameters>);          -> protos["gkg_name"] = (restype, argtypes): a pointer to a struct of the header is
                                            POINTER(that struct), every other pointer c_void_p (callers pass raw device addresses)
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os
import re

from ._build import INCLUDE

HEADER = os.path.join(INCLUDE, "gkg_hip.h")


class GkgError(RuntimeError):
    pass


# constants: name without GKG_ -> int; structs: C name -> Structure subclass; protos: entry point -> (restype, [argtypes]) — all three
# dicts in declaration order
Abi = collections.namedtuple("Abi", "constants structs protos")

_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "long": C.c_long, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
            "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_RETURNS = {**_SCALARS, "void": None, "const char*": C.c_char_p}
_DECL = re.compile(r"(?:const\s+)?(\w[\w ]*?)\s*(\*|\s)\s*(\w+)")          # [const] <type> [*] <name>


def _decl(text, structs, param):
    """One declarator ``[const] type [*] name`` -> (name, ctype)."""
    m = _DECL.fullmatch(text.strip())
    if m is None:
        raise GkgError(f"gkg_hip.h: cannot parse the declaration {text.strip()!r}")
    base, ptr, name = m.group(1), m.group(2) == "*", m.group(3)
    if ptr:
        return name, (C.POINTER(structs[base]) if param and base in structs else C.c_void_p)
    if base not in structs and base not in _SCALARS:
        raise GkgError(f"gkg_hip.h: no ctypes mapping for the type {base!r} in {text.strip()!r}")
    return name, structs.get(base) or _SCALARS[base]


def _fields(body, structs):
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        first, *more = stmt.split(",")
        if more and "*" in stmt:
            raise GkgError(f"gkg_hip.h: several declarators in a pointer declaration: {stmt!r}")
        name, ctype = _decl(first, structs, False)
        if not all(re.fullmatch(r"\s*\w+\s*", n) for n in more):
            raise GkgError(f"gkg_hip.h: cannot parse the declaration {stmt!r}")
        fields += [(n.strip(), ctype) for n in [name] + more]
    return fields


def _restype(text):
    text = re.sub(r"\s*\*", "*", " ".join(text.split()))
    if text not in _RETURNS:
        raise GkgError(f"gkg_hip.h: no ctypes mapping for the return type {text!r}")
    return _RETURNS[text]


def parse(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//.*", " ", text)
    declared = set(re.findall(r"\b(gkg_[a-z_0-9]+)\s*\(", text))
    constants, structs, protos = {}, {}, {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+GKG_(\w+)(.*)$", text, flags=re.M):
        if value.strip():
            try:
                constants[name] = int(re.sub(r"[uU]$", "", value.strip()), 0)
            except ValueError:
                raise GkgError(f"gkg_hip.h: #define GKG_{name}{value.rstrip()} is not an integer literal") from None
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    def struct(m):
        structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": _fields(m.group(2), structs)})
        return ""
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", struct, text, flags=re.S)
    left = re.search(r"\b(typedef|struct|union|enum)\b.*", text)
    if left:
        raise GkgError(f"gkg_hip.h: only `typedef struct X {{ ... }} X;` is understood, not {left.group(0)!r}")
    for ret, name, params in re.findall(r"([\w \t*]+?)\b(gkg_\w+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        args = [] if params in ("", "void") else [_decl(p, structs, True)[1] for p in params.split(",")]
        protos[name] = (_restype(ret), args)
    if set(protos) != declared:
        raise GkgError(f"gkg_hip.h: {len(declared)} entry points named, {len(protos)} prototypes bound; "
                       f"not parsed: {sorted(declared - set(protos))}")
    return Abi(constants, structs, protos)


@functools.lru_cache(maxsize=None)
def header():
    """include/gkg_hip.h, parsed once per process."""
    try:
        with open(HEADER) as fh:
            text = fh.read()
    except OSError as e:
        raise GkgError(f"{HEADER} not found ({e.strerror}): the Python binding is derived from it") from None
    return parse(text)


def bind(lib):
    """restype / argtypes of every entry point the header declares, on a loaded library."""
    for name, (restype, argtypes) in header().protos.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise GkgError(f"{name} is declared in gkg_hip.h but not exported by the library; rebuild") from None
        fn.restype, fn.argtypes = restype, argtypes
