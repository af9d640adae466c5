"""The environment switches of the main library, stated once in lidar-gs_amd/csrc/switches.h: tests/switches_probe.cpp (a plain C++
program around that header: no GPU, no HIP) prints what it reads under controlled environments, and the expectations below are the
rules written out by hand.  Two source checks: no other file of csrc/ reads the environment, and README's table names the same switches."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-gs_amd", "csrc")
P = "LIDARGS_"

# the probe's output in an environment without any switch (booleans as 0 / 1; NG_T16_PASSES as the number of passes)
DEFAULTS = dict(TILE_ROWS="0", SEG_LEN="0", MAX_SEGMENTS="0", ROUNDS="unset", HEAD="-1", FUSED="-1", RANGE_SORT_BITS="8", NO_PRUNE="0",
                TILE_KEY32="0", NO_SMALL_SORT="0", SMALL_SORT_MAX="4096", RANGE_SORT_FULL="0", NG_PER_LANE_DECODE="0", CHAMFER_BRUTE="0",
                WORK_LISTS="1", RANGE_SORT_BUCKETS="1", RANGE_SORT_PACKED="1", WALK2="7", FUSED_WAVES="8", P2_GROUP="0", SORT_ITEMS="0",
                DETERMINISTIC="0", NG_FORWARD_T16="1", NG_BACKWARD_T16="1", NG_T16_PASSES="2", NG_T16_STAGGER="0", RANGE_SORT_BUCKET_BITS="0")
# switch: [(value it is set to, what the probe then prints for it)]: an accepted value, each boundary, a rejected value
RULES = {
    "TILE_ROWS": [("4", "4"), ("8", "8"), ("16", "16"), ("32", "32"), ("5", "0"), ("64", "0"), ("", "0")],
    "SEG_LEN": [("128", "128"), ("64", "64"), ("10", "64"), ("-5", "64"), ("", "64")],
    "MAX_SEGMENTS": [("33", "33"), ("44", "45"), ("0", "1"), ("1", "1"), ("63", "63"), ("64", "63"), ("-2", "1")],
    "ROUNDS": [("2,6", "2,6"), ("3,3,9", "3,9"), ("9,3", "9"), ("300,5", "5"), ("", ""), ("0", ""), ("1,2,3,4,5,6,7,8,9,10", "1,2,3,4,5,6,7,8"),
               ("2,6,", "2,6"), ("5,", "5"), ("a,4", "4"), ("254,255", "254"), (",,7", "7")],
    "HEAD": [("0", "0"), ("1", "1"), ("-1", "-1"), ("3", "3")],           # (plan_segments takes any value >= 0, non-zero as 1)
    "FUSED": [("0", "0"), ("1", "1"), ("-1", "-1")],
    "RANGE_SORT_BITS": [("8", "8"), ("11", "11"), ("12", "8"), ("7", "8")],
    "SMALL_SORT_MAX": [("100", "100"), ("0", "0"), ("-1", "0"), ("16384", "16384"), ("16385", "16384"), ("99999999999999", "16384")],
    "WALK2": [("0", "0"), ("5", "5"), ("7", "7")],
    "FUSED_WAVES": [("4", "4"), ("16", "16"), ("8", "8"), ("5", "8")],
    "P2_GROUP": [("3", "3"), ("0", "0"), ("-3", "0"), ("64", "64"), ("99", "64")],
    "SORT_ITEMS": [("8", "8"), ("16", "16"), ("0", "0")],
    "DETERMINISTIC": [("", "0"), ("0", "0"), ("1", "1"), ("yes", "0")],
    "NG_FORWARD_T16": [("00", "0"), ("0x", "0"), ("0", "0"), ("1", "1"), ("", "1")],
    "NG_BACKWARD_T16": [("0", "0"), ("1", "1"), ("x0", "1")],
    "NG_T16_PASSES": [("1", "1"), ("10", "1"), ("2", "2"), ("", "2")],
    "NG_T16_STAGGER": [("3", "3"), ("0", "0")],
    "RANGE_SORT_BUCKET_BITS": [("10", "10"), ("11", "11"), ("12", "0"), ("9", "0")],     # (the probe hands in the widths 10 and 11)
}
for _name in ("NO_PRUNE", "TILE_KEY32", "NO_SMALL_SORT", "RANGE_SORT_FULL", "NG_PER_LANE_DECODE", "CHAMFER_BRUTE"):      # off unless atoi != 0
    RULES[_name] = [("1", "1"), ("2", "1"), ("0", "0"), ("", "0"), ("on", "0")]
for _name in ("WORK_LISTS", "RANGE_SORT_BUCKETS", "RANGE_SORT_PACKED"):                                                    # on unless atoi == 0
    RULES[_name] = [("0", "0"), ("", "0"), ("1", "1"), ("-1", "1")]
CASES = [({}, {})] + [({name: value}, {name: want}) for name, rule in RULES.items() for value, want in rule] + [
    ({"FUSED": "0", "WORK_LISTS": "0", "HEAD": "1"}, {"FUSED": "0", "WORK_LISTS": "0", "HEAD": "1"}),
    ({"NO_SMALL_SORT": "1", "SMALL_SORT_MAX": "16384"}, {"NO_SMALL_SORT": "1", "SMALL_SORT_MAX": "16384"})]


@pytest.fixture(scope="session")
def probes(tmp_path_factory):
    """The probe, plain and with the address and undefined-behaviour sanitizers (host code in a program of its own; their runtimes linked
    statically, so that the program does not depend on the order its libraries are loaded in)."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("switches")
    built = {}
    sanitize = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    for name, flags in (("plain", ["-O1"]), ("sanitized", ["-O1"] + sanitize)):
        exe = str(d / name)
        subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "switches_probe.cpp"), "-o", exe], check=True)
        built[name] = exe
    return built


def probe(exe, env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith(P)}
    r = subprocess.run([exe], env=dict(clean, **{P + k: v for k, v in env.items()}), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (env, r.stderr[-3000:])
    return dict(line[len(P):].split("=", 1) for line in r.stdout.splitlines())


def test_the_empty_environment_gives_every_default(probes):
    assert probe(probes["plain"], {}) == DEFAULTS and len(DEFAULTS) == 27


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_every_rule_of_the_table(build, probes):
    """Each case changes exactly the switches it sets; under the sanitizers the same list once more (LIDARGS_ROUNDS is parsed by hand)."""
    assert set(RULES) == set(DEFAULTS)
    for env, want in CASES:
        assert probe(probes[build], env) == dict(DEFAULTS, **want), env


def test_only_switches_h_reads_the_environment():
    readers = [f for f in sorted(os.listdir(CSRC)) if "getenv" in open(os.path.join(CSRC, f), errors="replace").read()]
    assert readers == ["switches.h"]


def test_readme_table_and_code_name_the_same_switches(probes):
    readme = open(os.path.join(ROOT, "README.md")).read()
    table = readme[readme.index("Environment switches"):]
    rows = list(itertools.takewhile(lambda line: line.startswith("|") or not line.strip(), table.splitlines()[1:]))
    in_table = set(re.findall(r"LIDARGS_[A-Z0-9_]+", "\n".join(rows)))
    printed = {P + k for k in probe(probes["plain"], {})}
    python = [os.path.join(d, f) for d, _, files in os.walk(os.path.join(ROOT, "lidar-gs_amd")) for f in files if f.endswith(".py")]
    literals, read = set(), set()
    for path in python + [os.path.join(ROOT, "bench.py")]:
        text = open(path).read()
        literals |= set(re.findall(r"""["'](LIDARGS_[A-Z0-9_]+)["']""", text))
        if path in python:
            read |= set(re.findall(r"""os\.environ\.get\(\s*["'](LIDARGS_[A-Z0-9_]+)["']""", text))
    assert printed - in_table == set(), "switches of csrc/switches.h without a row in README"
    assert in_table - printed - literals == set(), "README rows that name no switch of the code"
    assert read - in_table == set(), "switches the Python side reads without a row in README"
    assert len(read) >= 7 and len(in_table) >= len(printed) + len(read)
