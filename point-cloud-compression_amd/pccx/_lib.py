"""ctypes loader for libpccx.so (the C ABI declared in include/pccx.h).

There is NO CPU fallback: if the library is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os
import re

from .build import INCLUDE

_HERE = os.path.dirname(os.path.abspath(__file__))
# PCCX_LIB: another build of the same ABI (a sanitizer or experiment build).  PCCX_LIB_PARTIAL=1 accepts a library that exports only
# part of the ABI -- the host-only sanitizer build of the packers (oracle/Makefile `asan`); calling an entry point it lacks raises.
LIB_PATH = os.environ.get("PCCX_LIB") or os.path.join(_HERE, "lib", "libpccx.so")

HEADER = os.path.join(INCLUDE, "pccx.h")

_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_DECL = re.compile(r"PCCX_API\s+([\w\s*]+?)\b(pccx_\w+)\s*\(([^()]*)\)\s*;")

_lib = None
_signatures = None


class PccxError(RuntimeError):
    pass


def _ctype(decl, name, named):
    """ctypes type of one return type (named=False) or one parameter declaration of pccx.h.  Device pointers travel as integers
    (tensor.data_ptr()), so every pointer is a c_void_p except the host strings."""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return C.c_char_p if words[:3] == ["const", "char", "*"] else C.c_void_p
    words = [w for w in words if w != "const"]
    if named and len(words) == 2:
        words.pop()
    if len(words) != 1 or words[0] not in _SCALARS:
        raise PccxError(f"pccx.h: {name}: no ctypes mapping for {decl.strip()!r}")
    return _SCALARS[words[0]]


def parse_header(text):
    """name -> (restype, argtypes) of every PCCX_API declaration in ``text``; an unknown type raises, it is never taken as int."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    table = {}
    for decl in re.findall(r"^\s*(PCCX_API\b[^;]*;)", text, flags=re.M):
        m = _DECL.fullmatch(decl)
        if m is None:
            raise PccxError(f"pccx.h: cannot read the declaration {' '.join(decl.split())!r}")
        ret, name, args = m.groups()
        params = [] if args.strip() in ("", "void") else args.split(",")
        table[name] = (_ctype(ret, name, False), [_ctype(p, name, True) for p in params])
    return table


def signatures():
    global _signatures
    if _signatures is None:
        with open(HEADER) as f:
            _signatures = parse_header(f.read())
    return _signatures


def load():
    """Load libpccx.so and type every entry point from include/pccx.h; raises PccxError when the library has not been built
    (python -m pccx.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PccxError(
                f"{LIB_PATH} not found: build the HIP library first (python -m pccx.build). "
                "pccx has no CPU fallback.")
        # torch first: its bundled HIP runtime must be the one (and only) libamdhip64 in the process,
        # so that libpccx's kernels and torch's allocator / streams share devices and contexts.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        partial = os.environ.get("PCCX_LIB_PARTIAL") == "1"
        for name, (restype, argtypes) in signatures().items():
            if partial and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)   # AttributeError if the library and the header disagree
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = lib
    return _lib


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise PccxError(f"{name} failed ({rc}): {lib.pccx_last_error().decode()}")


def declared_symbols():
    return list(signatures())
