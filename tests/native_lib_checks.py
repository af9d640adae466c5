"""The checks every library of build_hip.TARGETS but the main one gets, stated once: each of them is a single source with a header
directory of its own, and its CPU test file calls check_library() with the functions it expects that header to declare."""
import os
import re
import subprocess

import build_hip
import lidargs_abi

# target name -> "test module:its set of declared functions": the module whose test calls check_library() for that target
SATELLITES = {"optim": "test_optim_cpu:DECLARED", "decode_options": "test_decode_options_cpu:NEW", "tcnn": "test_tcnn_cpu:DECLARED",
              "rangeview": "test_range_view_cpu:DECLARED", "scatter": "test_scatter_cpu:DECLARED"}


def exports(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r" T (lidargs_\w+)", out))


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
