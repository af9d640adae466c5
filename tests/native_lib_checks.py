"""The checks every library of build_hip.TARGETS but the main one gets, stated once: each of them is a single source with a header
directory of its own, and its CPU test file calls check_library() with the functions it expects that header to declare.  The main
library's families of further entry points get check_family() in the same way."""
import os
import re
import subprocess

import pytest

import build_hip
import lidargs_abi

# target name -> "test module:its set of declared functions": the module whose test calls check_library() for that target
SATELLITES = {"optim": "test_optim_cpu:DECLARED", "decode_options": "test_decode_options_cpu:NEW", "tcnn": "test_tcnn_cpu:DECLARED",
              "rangeview": "test_range_view_cpu:DECLARED", "scatter": "test_scatter_cpu:DECLARED"}
# family of TARGETS["hip"] -> "test module:its set of declared functions": the module whose test calls check_family() for that family
FAMILIES = {"pose": "test_pose_abi_cpu:DECLARED", "surfel_pose": "test_surfel_pose_abi_cpu:DECLARED", "sweep": "test_sweep_abi_cpu:DECLARED"}


def exports(so, prefix="lidargs"):
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r" T (%s_\w+)" % prefix, out))


def check_library(target, declared, lib, main_so):
    """`target` was built from sources of its own, its header directory declares exactly `declared` in plain C, its library exports
    exactly that and nothing the main library (`main_so`) exports, and every function of the loaded CDLL `lib` is typed as the header
    says.  Returns lidargs_abi's signatures of the header directory."""
    assert target is build_hip.TARGETS[target.name] and target.name in SATELLITES
    assert os.path.exists(target.out), "build_hip.build() must build every library of TARGETS"
    assert target.sources and not set(target.sources) & set(build_hip.SOURCES)
    typed = lidargs_abi.signatures(target.include)
    assert set(typed) == declared
    exported = exports(target.out)
    assert exported - declared == set(), "exported but not declared in " + target.include
    assert declared - exported == set(), "declared in " + target.include + " but not exported"
    assert exports(main_so).isdisjoint(declared)
    for name, (restype, argtypes) in typed.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == argtypes, name
    for h in sorted(os.listdir(target.include)):
        r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-x", "c", os.path.join(target.include, h)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return typed


def check_family(name, header, declared, main_so):
    """The family `name` of the main library: its directory holds `header` alone, which is plain C and declares exactly `declared` under the
    family's prefix and nothing under another prefix of the library; the library (`main_so`) exports exactly that under the prefix, and
    under `lidargs_` still exactly what include/ declares; the header is hashed, and rebuilt for by the main library alone; and every
    function is typed on the process' one CDLL as the header says.  Returns lidargs_abi's signatures of the family."""
    from test_abi_cpu import INSTRUMENTED_ONLY
    hip = build_hip.TARGETS["hip"]
    family = {f.name: f for f in hip.families}[name]
    assert name in FAMILIES and os.listdir(family.include) == [header]
    header = os.path.join(family.include, header)
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-x", "c", header], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    typed = lidargs_abi.signatures(family.include, family.prefix)
    assert set(typed) == declared
    for other in [hip.prefix] + [f.prefix for f in hip.families if f is not family]:      # nothing of another family hides in this directory
        with pytest.raises(ImportError):
            lidargs_abi.signatures(family.include, other)
    assert exports(main_so, family.prefix) == declared
    assert exports(main_so) - INSTRUMENTED_ONLY == set(lidargs_abi.signatures())             # the drop-in boundary is what include/ declares
    assert header in build_hip.deps(hip) and header in build_hip.build_id_files()            # the library is rebuilt for it
    assert not any(header in build_hip.deps(t) for t in build_hip.TARGETS.values() if t is not hip)
    from diff_lidargs_rasterization import _C
    for fn, (restype, argtypes) in typed.items():
        assert getattr(_C._lib, fn).restype is restype and tuple(getattr(_C._lib, fn).argtypes) == argtypes, fn
    return typed
