"""CPU tests of build_hip's table of targets: what a library is rebuilt for, what the build id hashes and what a second build does,
for every target at once; and that every library beside the main one, and every family of further entry points in the main one, has a
test file that checks it against its header."""
import importlib
import os

import build_hip
import lidargs_abi
from native_lib_checks import FAMILIES, SATELLITES

TARGETS = build_hip.TARGETS
SCRIPT = os.path.abspath(build_hip.__file__)


def headers(t):
    return [os.path.join(d, h) for d in build_hip.header_dirs(t) for h in os.listdir(d)]


def test_table_is_ordered_and_every_satellite_has_its_checks():
    assert list(TARGETS) == ["hip", "optim", "decode_options", "tcnn", "rangeview", "scatter"] and all(t.name == k for k, t in TARGETS.items())
    assert TARGETS["hip"].out == build_hip.OUT and TARGETS["hip"].sources is build_hip.SOURCES
    assert len({t.out for t in TARGETS.values()}) == len({t.include for t in TARGETS.values()}) == len(TARGETS)
    dirs = [d for t in TARGETS.values() for d in build_hip.header_dirs(t)]
    assert len(set(dirs)) == len(dirs) and all(build_hip.header_dirs(t)[0] == t.include for t in TARGETS.values())
    assert set(SATELLITES) == set(TARGETS) - {"hip"}, "a library of TARGETS without a registered declared set"
    for name, where in SATELLITES.items():
        module, attr = where.split(":")
        assert getattr(importlib.import_module(module), attr) == set(lidargs_abi.signatures(TARGETS[name].include)), name


def test_families_are_the_main_library_s_and_every_family_has_its_checks():
    assert [f.name for f in TARGETS["hip"].families] == ["pose", "surfel_pose", "sweep"]
    assert all(t.families == () for t in TARGETS.values() if t.name != "hip")
    assert list(FAMILIES) == [f.name for f in TARGETS["hip"].families], "a family of TARGETS without a registered declared set"
    for f in TARGETS["hip"].families:
        module, attr = FAMILIES[f.name].split(":")
        assert getattr(importlib.import_module(module), attr) == set(lidargs_abi.signatures(f.include, f.prefix)), f.name
    # a prefix is written without its underscore; no two are alike, and no family's names begin as another prefix's do or the reverse
    prefixes = [t.prefix for t in TARGETS.values()] + [f.prefix for t in TARGETS.values() for f in t.families]
    assert len(set(prefixes)) == len(prefixes) and not [p for p in prefixes if p.endswith("_")]
    for f in TARGETS["hip"].families:
        for p in prefixes:
            assert p == f.prefix or not ((f.prefix + "_").startswith(p + "_") or (p + "_").startswith(f.prefix + "_")), (f.prefix, p)


def test_deps_hold_the_sources_the_headers_and_the_build_script():
    shared = [os.path.join(build_hip.CSRC, f) for f in os.listdir(build_hip.CSRC) if not f.endswith(".hip")]
    assert shared, "csrc/ holds headers that the sources include"
    for t in TARGETS.values():
        d = build_hip.deps(t)
        assert all(os.path.exists(f) for f in d)
        assert set(d) >= {os.path.join(build_hip.CSRC, s) for s in t.sources} | set(headers(t)) | set(shared) | {SCRIPT}, t.name
    main = build_hip.deps(TARGETS["hip"])
    assert not [s for t in TARGETS.values() if t.name != "hip" for s in t.sources if os.path.join(build_hip.CSRC, s) in main]
    assert os.path.join(TARGETS["hip"].include, "lidargs_loss.h") in main                  # not lidargs_rasterizer.h alone
    in_table = {s for t in TARGETS.values() for s in t.sources}
    assert in_table == {f for f in os.listdir(build_hip.CSRC) if f.endswith(".hip")}       # every source belongs to a target


def test_build_id_hashes_csrc_every_header_directory_and_the_build_script():
    files = build_hip.build_id_files()
    assert len(files) == len(set(files)) and files == build_hip.build_id_files()           # the same list in the same order every time
    want = {os.path.join(build_hip.CSRC, f) for f in os.listdir(build_hip.CSRC)} | {SCRIPT}
    for t in TARGETS.values():
        want |= set(headers(t))
    assert set(files) == want
    assert build_hip.build_id() == build_hip.build_id() and len(build_hip.build_id()) == 12


def test_nothing_is_stale_after_a_build_and_a_second_build_links_nothing(hip_lib_built):
    assert not [t.name for t in TARGETS.values() if build_hip.stale(t)]
    before = {t.name: os.stat(t.out).st_mtime_ns for t in TARGETS.values()}
    assert os.path.abspath(build_hip.build()) == os.path.abspath(hip_lib_built)
    assert {t.name: os.stat(t.out).st_mtime_ns for t in TARGETS.values()} == before
