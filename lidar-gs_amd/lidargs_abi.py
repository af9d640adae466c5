"""lidargs_abi -- the Python side of the C ABI: one loader, every signature read from the public headers.

`load(path)` opens liblidargs_hip.so and sets `restype` and `argtypes` of every function the headers under include/ declare; the
result is the one `CDLL` every module calls through (`diff_lidargs_rasterization._C._lib`).  A second library with a header directory
and a version function of its own (liblidargs_optim.so, include_optim/) is loaded by the same function with those three named.  The headers are the only source: a new
entry point is typed the moment it is declared, and a prototype this parser cannot map is an ImportError naming the function, never
a function left untyped.

The argtypes are plain ctypes types (no Python-level `from_param`, no wrapper around the functions), so call sites pass plain Python
numbers for `int` / `float` / `double` / `size_t` parameters and `c_void_p` (or None) for every pointer and allocator callback.
ctypes then refuses, before the library is entered:
    too few arguments                                              TypeError
    a float, or a pointer object (`_ptr(t)`), in an int / size_t slot    ctypes.ArgumentError
    a float or a c_int in a pointer slot                           ctypes.ArgumentError
    a ctypes instance of another type than declared (c_int for size_t)   ctypes.ArgumentError
It does NOT refuse surplus arguments (ctypes passes them on) or a bare Python int in a pointer slot (c_void_p takes an address):
pointers therefore travel as `c_void_p` objects, so that a spliced argument list that is one too long or too short still fails
wherever the shift puts a pointer object into a scalar slot.
"""
import ctypes as C
import os
import re

INCLUDE = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include"))
ABI_VERSION = 2     # LIDARGS_ABI_VERSION of include/lidargs_rasterizer.h

_BY_VALUE = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_RETURNS = dict(_BY_VALUE, **{"void": None, "const char*": C.c_char_p})
_PROTOTYPE = re.compile(r"(?P<ret>[\w\s*]+?)\s*\b(?P<name>lidargs_\w+)\s*\((?P<params>.*)\)", re.S)


def _split_params(params):
    """Split at the commas of parenthesis depth 0 (a function-pointer parameter declared inline has commas of its own)."""
    out, depth, cur = [], 0, ""
    for ch in params:
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            out.append(cur); cur = ""
        else:
            cur += ch
    return [p.strip() for p in out + [cur]]


def _param_type(decl, name):
    """Every pointer, function pointers and lidargs_alloc_fn included, is a c_void_p: it takes None, c_void_p, ctypes arrays,
    byref(...) and CFUNCTYPE instances alike.  What is passed by value must be one of the four scalar types."""
    if "*" in decl or decl.split()[0] == "lidargs_alloc_fn":
        return C.c_void_p
    ctype = _BY_VALUE.get(" ".join(decl.split()[:-1]))      # (the last word is the parameter's name)
    if ctype is None:
        raise ImportError(f"lidargs_abi: cannot map parameter `{decl}` of {name}")
    return ctype


def parse_header(text):
    """{function name: (restype, (argtypes, ...))} of every prototype in a header's text.  Comments, preprocessor lines, typedefs,
    enums and the extern "C" braces are dropped; every statement that is left must be a `lidargs_*` prototype."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    src = re.sub(r"^[ \t]*#.*$", " ", src, flags=re.M)
    src = re.sub(r"\b(typedef|enum)\b[^;{]*(\{[^}]*\})?[^;]*;", " ", src)
    src = re.sub(r'extern\s+"C"\s*\{', " ", src).replace("}", " ")
    sigs = {}
    for stmt in filter(None, (s.strip() for s in src.split(";"))):
        m = _PROTOTYPE.fullmatch(stmt)
        if m is None:
            raise ImportError(f"lidargs_abi: cannot parse the declaration `{' '.join(stmt.split())[:120]}`")
        name, ret = m["name"], re.sub(r"\s*\*", "*", " ".join(m["ret"].split()))
        if ret not in _RETURNS:
            raise ImportError(f"lidargs_abi: cannot map the return type `{ret}` of {name}")
        params = _split_params(m["params"])
        sigs[name] = (_RETURNS[ret], () if params == ["void"] else tuple(_param_type(p, name) for p in params))
    return sigs


def signatures(include=INCLUDE):
    """The signatures of every header of a header directory (include/ unless another is named)."""
    if not os.path.isdir(include):
        raise ImportError(f"lidargs_abi: the public headers ({include}) are missing; the binding reads its signatures from them")
    sigs = {}
    for fn in sorted(f for f in os.listdir(include) if f.endswith(".h")):
        with open(os.path.join(include, fn)) as f:
            sigs.update(parse_header(f.read()))
    return sigs


def load(path, include=INCLUDE, version_fn="lidargs_abi_version", version=ABI_VERSION, package="diff_lidargs_rasterization"):
    """The typed CDLL of the library at `path` (liblidargs_hip.so unless the other arguments say otherwise): every function the headers
    of `include` declare is typed, and `version_fn()` must return `version`.  `package` names the importer in the error messages."""
    so = os.path.basename(path)
    if not os.path.exists(path):
        raise ImportError(
            f"{package}: native library {path} is missing. Build it with "
            "`python lidar-gs_amd/build_hip.py` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in signatures(include).items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError(f"{package}: {so} does not export {name}, which the headers declare; rebuild it") from None
        fn.restype, fn.argtypes = restype, argtypes
    if getattr(lib, version_fn)() != version:
        raise ImportError(f"{package}: {so} ABI version mismatch; rebuild it")
    return lib
