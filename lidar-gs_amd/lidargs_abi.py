"""lidargs_abi -- the Python side of the C ABI: one loader, every signature and integer constant read from the public headers.

`library(name)` opens the library of `build_hip.TARGETS[name]` and sets `restype` and `argtypes` of every function its header directories
declare, the primary one and those of its families alike; for "hip" the result is the one `CDLL` every module calls through
(`diff_lidargs_rasterization._C._lib`).  The table says where the library and its headers are, how its symbols begin and which package
the error messages name; `load()` is the same with these spelt out.  A prefix is written as the table writes it, without the underscore
that ends it (`lidargs`, `lgpose`); `_prototype` alone adds it.
The headers are the only source: a new entry point is typed the moment it is declared, a prototype this parser cannot map is
an ImportError naming the function, never a function left untyped, and the expected ABI version and every other `#define LIDARGS_*
<integer>` is read (`constants`), not mirrored.  What every call site needs around a call is here once as well: `ptr`, `stream`, `check`
and `poison_scratch`.

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

import torch

import build_hip

INCLUDE = build_hip.TARGETS["hip"].include

_BY_VALUE = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_RETURNS = dict(_BY_VALUE, **{"void": None, "const char*": C.c_char_p})
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_CONSTANT = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(LIDARGS_\w+)[ \t]+(-?\d+|\(-?\d+\))[ \t]*$", re.M)


def _prototype(prefix):
    """A whole statement that declares a function named <prefix>_* (re keeps what it compiled)."""
    return re.compile(r"(?P<ret>[\w\s*]+?)\s*\b(?P<name>" + re.escape(prefix) + r"_\w+)\s*\((?P<params>.*)\)", re.S)


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


def parse_header(text, prefix="lidargs"):
    """{function name: (restype, (argtypes, ...))} of every prototype in a header's text.  Comments, preprocessor lines, typedefs,
    enums and the extern "C" braces are dropped; every statement that is left must be a `lidargs_*` prototype (`prefix`: another
    family of names, as the pose header's `lgpose`)."""
    prototype = _prototype(prefix)
    src = _COMMENT.sub(" ", text)
    src = re.sub(r"^[ \t]*#.*$", " ", src, flags=re.M)
    src = re.sub(r"\b(typedef|enum)\b[^;{]*(\{[^}]*\})?[^;]*;", " ", src)
    src = re.sub(r'extern\s+"C"\s*\{', " ", src).replace("}", " ")
    sigs = {}
    for stmt in filter(None, (s.strip() for s in src.split(";"))):
        m = prototype.fullmatch(stmt)
        if m is None:
            raise ImportError(f"lidargs_abi: cannot parse the declaration `{' '.join(stmt.split())[:120]}`")
        name, ret = m["name"], re.sub(r"\s*\*", "*", " ".join(m["ret"].split()))
        if ret not in _RETURNS:
            raise ImportError(f"lidargs_abi: cannot map the return type `{ret}` of {name}")
        params = _split_params(m["params"])
        sigs[name] = (_RETURNS[ret], () if params == ["void"] else tuple(_param_type(p, name) for p in params))
    return sigs


def _headers(include):
    """The text of every header of a header directory, in the order of their names."""
    if not os.path.isdir(include):
        raise ImportError(f"lidargs_abi: the public headers ({include}) are missing; the binding reads its signatures from them")
    for fn in sorted(f for f in os.listdir(include) if f.endswith(".h")):
        with open(os.path.join(include, fn)) as f:
            yield f.read()


def signatures(include=INCLUDE, prefix="lidargs"):
    """The signatures of every header of a header directory (include/ unless another is named)."""
    sigs = {}
    for text in _headers(include):
        sigs.update(parse_header(text, prefix))
    return sigs


def constants(include=INCLUDE):
    """{name: int} of every `#define LIDARGS_* <integer>` of a header directory: a decimal integer, in parentheses or not, and nothing
    behind it but a comment.  A #define of anything else (an include guard, an expression) is not a constant and is left out."""
    return {name: int(body.strip("()")) for text in _headers(include) for name, body in _CONSTANT.findall(_COMMENT.sub(" ", text))}


def __getattr__(name):
    if name == "ABI_VERSION":           # of include/, read when asked for: a tree without headers still imports and says so in load()
        return constants(INCLUDE)["LIDARGS_ABI_VERSION"]
    raise AttributeError(f"module 'lidargs_abi' has no attribute '{name}'")


def load(path, include=INCLUDE, version_fn="lidargs_abi_version", version=None, package="diff_lidargs_rasterization", families=()):
    """The typed CDLL of the library at `path` (liblidargs_hip.so unless the other arguments say otherwise): every function the headers
    of `include` declare, and of each of `families` (build_hip.Family: a header directory and the prefix of its names), is typed, and
    `version_fn()` must return `version`: unless one is given, the macro of that name in upper case (LIDARGS_ABI_VERSION), as the
    headers define it.  `package` names the importer in the error messages."""
    so = os.path.basename(path)
    if not os.path.exists(path):
        raise ImportError(
            f"{package}: native library {path} is missing. Build it with "
            "`python lidar-gs_amd/build_hip.py` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    sigs = signatures(include)
    for family in families:
        sigs.update(signatures(family.include, family.prefix))
    for name, (restype, argtypes) in sigs.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError(f"{package}: {so} does not export {name}, which the headers declare; rebuild it") from None
        fn.restype, fn.argtypes = restype, argtypes
    if version is None:
        version = constants(include)[version_fn.upper()]
    if getattr(lib, version_fn)() != version:
        raise ImportError(f"{package}: {so} ABI version mismatch; rebuild it")
    lib.last_error = getattr(lib, version_fn[:-len("abi_version")] + "last_error")       # what check() reads
    return lib


def library_constants(name):
    """constants() of the header directory of the library `name` of build_hip.TARGETS."""
    return constants(build_hip.TARGETS[name].include)


def library(name):
    """load() of the library `name` of build_hip.TARGETS, with everything taken from its entry."""
    t = build_hip.TARGETS[name]
    return load(t.out, include=t.include, version_fn=t.prefix + "_abi_version", package=t.package, families=t.families)


def ptr(t):
    """Device pointer of a tensor; NULL for None and for an empty tensor (torch gives data_ptr() == 0 for one, which is what the
    reference relies on for `cov3D_precomp != nullptr`, R3/cr/forward.cu:307)."""
    if t is None or t.numel() == 0:
        return None
    return C.c_void_p(t.data_ptr())


def stream(device_or_tensor):
    """The current HIP stream of a device, or of a tensor's."""
    return C.c_void_p(torch.cuda.current_stream(getattr(device_or_tensor, "device", device_or_tensor)).cuda_stream)


def check(lib, rc, what):
    """A negative return code of a call into `lib` is a RuntimeError that carries the library's own message."""
    if rc < 0:
        raise RuntimeError(f"{what} failed with code {rc}: {lib.last_error().decode(errors='replace')}")


def poison_scratch():
    """LIDARGS_POISON_SCRATCH=1 (tests): every scratch buffer handed to a library is filled with 0xFF bytes (NaN floats, huge integers)
    first, so that a kernel reading scratch memory nobody wrote shows up deterministically instead of depending on what the caching
    allocator happens to recycle."""
    return os.environ.get("LIDARGS_POISON_SCRATCH", "0") == "1"
