"""The C ABI's prototypes for ctypes, read from include/htk_amd.h: the header is the one statement of the ABI.

The header is plain C with a small vocabulary -- scalars, pointers to them, typedef'd structs and opaque handles, no function
pointers -- so a few regular expressions parse it.  Anything outside that vocabulary is an error here, never a silent C int.

Mapping: scalars to their ctypes scalar; `const char *` to c_char_p; every other pointer PARAMETER (out-buffers, T **, struct
pointers, handles, streams, arrays) to c_void_p, which takes what callers pass: data_as(c_void_p), byref(), ctypes arrays, None and
the plain integer of a tensor's data_ptr().  Pointer RETURNS: `const float *` to POINTER(c_float), a pointer to a struct to
POINTER(its ctypes mirror), an opaque handle to c_void_p.
"""
from __future__ import annotations

import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "htk_amd.h")

SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long": C.c_long, "long long": C.c_longlong, "size_t": C.c_size_t}
_POINTEES = set(SCALARS) | {"void", "char", "unsigned char", "short"}      # what a pointer may point to, besides the header's own types
_STRUCT = r"typedef\s+struct\s*\{[^{}]*\}\s*(\w+)\s*;"
_HANDLE = r"typedef\s+struct\s+\w+\s+(\w+)\s*;"


def _code(text: str) -> str:
    """The header without comments, preprocessor lines (continuations included) and the extern "C" brace."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", "", text, flags=re.M)
    return re.sub(r'extern\s+"C"\s*\{', "", text)


def struct_names(text: str):
    """The names of the header's structs with a body (the ones that need a ctypes mirror)."""
    return re.findall(_STRUCT, _code(text))


def _ctype(decl: str, what: str, is_return: bool, structs: dict, own: set):
    tok = re.findall(r"\w+|\*|\[[^\]]*\]", decl)
    words = [t for t in tok if t[0] not in "*["]
    vocabulary = {"const", "unsigned"} | _POINTEES | own
    if len(words) > 1 and words[-1] not in vocabulary:      # the parameter's name
        words.pop()
    base = " ".join(w for w in words if w != "const")
    depth = len(tok) - len([t for t in tok if t[0] not in "*["])      # stars, and an array parameter is a pointer
    if depth == 0:
        if base == "void" and is_return:
            return None
        if base in SCALARS:
            return SCALARS[base]
    elif base in _POINTEES or base in own:
        if base == "char" and depth == 1 and words[0] == "const":
            return C.c_char_p
        if not is_return or (depth == 1 and base in own and base not in structs):      # a parameter, or an opaque handle
            return C.c_void_p
        if depth == 1 and base == "float":
            return C.POINTER(C.c_float)
        if depth == 1 and base in structs:
            return C.POINTER(structs[base])
    raise ValueError("htk_amd.h, %s: no ctypes mapping for '%s'" % (what, decl.strip()))


def prototypes(structs: dict, text: str = None) -> dict:
    """{function: (restype, [argtype, ...])} for every prototype of the header; `structs` maps a C struct's name to its ctypes mirror."""
    text = _code(open(HEADER).read() if text is None else text)
    own = set(re.findall(_STRUCT, text)) | set(re.findall(_HANDLE, text))
    missing = set(re.findall(_STRUCT, text)) - set(structs)
    if missing:
        raise ValueError("htk_amd.h: no ctypes mirror for %s" % sorted(missing))
    text = re.sub(_HANDLE, "", re.sub(_STRUCT, "", text))
    out = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):      # (the extern "C" brace's end)
            continue
        m = re.fullmatch(r"(.*?)\b(htkamd_\w+)\s*\((.*)\)", stmt)
        if not m or m.group(2) in out:
            raise ValueError("htk_amd.h: not a prototype, or a second one: '%s'" % stmt)
        ret, name, params = m.groups()
        args = [] if params.strip() == "void" else [_ctype(p, name, False, structs, own) for p in params.split(",")]
        out[name] = (_ctype(ret, name, True, structs, own), args)
    return out


def declare(L, structs: dict) -> None:
    """Set restype and argtypes of every declared function that the library exports (a build of the host code alone has no decoders)."""
    for name, (res, args) in prototypes(structs).items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
