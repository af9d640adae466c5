"""LIDARGS_DEPTH=second without a GPU: the restatement (tests/second_ref.py) on rays whose answer is known by arithmetic, the cap on
undecided pixels for every scene and gap the GPU tests use, the bound the second walk's early exit rests on, and the parse rules of the
switch and of LIDARGS_RETURN_GAP through a probe of this test's own around csrc/switches.h, plain and under the sanitizers, held
against the Python package's depth_mode() and return_gap() on one case list."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import median_ref as mr
import second_ref as s2
import strongest_ref as sr
from oracle import lgo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-gs_amd", "csrc")


@pytest.fixture(scope="module")
def restated():
    """{scene: (scene, W, strongest restatement, {gap: second restatement})}, once for the module."""
    out = {}
    for name in s2.SCENES:
        scene, W = s2.scene(name)
        f = lgo.forward(scene["means3D"], scene["colors"], scene["opacities"], scene["scales"], scene["rotations"], scene["viewmatrix"],
                        scene["beams"], W, s2.H, bg=scene["bg"])
        rs = sr.restate(f, scene, W, s2.H)
        out[name] = (scene, W, rs, {gap: s2.restate(f, rs, gap) for gap in s2.gaps(name)})
    return out


# The worked-out answers (range in m; 0 = no second return) at G = 0 and G = 0.505, from the nominal alphas 0.995 x opacity:
#   0.4/0.9              weights 0.40, 0.54: s = 20 m, the other is 10 m away
#   split surface        weights 0.50, 0.30, 0.18: s = 10.00 m; its neighbour at 10.02 m, or past the gap the wall
#   veil                 s = the wall (0.31); the layers' weights fall from 0.10: the first layer
#   thin                 s = layer 0; weights fall: layer 1 (10.01 m), or the first layer past the gap (10.51 m)
#   late wall            s = the wall (0.54, list position 100): layer 0
#   far second           weights 0.4975, 80 layers of at most 0.0025, the wall 0.8955 x 0.5025 x 0.995^80 = 0.30: s = 10 m, and the wall is
#                        the heaviest other entry at EITHER gap -- the rule's arithmetic, step 3.  (The layer at 10.01 m is the FIRST
#                        candidate at G = 0: the second walk carries best2 = 0.0025 past list position 64 and must not leave before the wall.)
ANSWERS = {"0.4/0.9": (10.0, 10.0), "split surface": (10.02, 20.0), "single": (0.0, 0.0), "pair inside the gap": (10.02, 0.0), "veil": (10.0, 10.0),
           "thin": (10.01, 10.51), "late wall": (10.0, 10.0), "far second": (20.0, 20.0), "first column": (12.0, 12.0), "last column": (10.0, 10.0),
           "nothing": (0.0, 0.0)}


@pytest.mark.parametrize("W", [64, 250, 256])
def test_hand_placed_rays(W, restated):
    scene, _, rs, by_gap = restated[f"second{W}"]
    for gap in s2.PLACED_GAPS:
        r = by_gap[gap]
        _, want, members = s2.placed(W, gap)
        t = r["table"]
        assert set(want) == set(ANSWERS)
        for case, (x, y, rng, gid) in want.items():
            assert r["decided"][y, x], (case, gap)
            assert r["second_id"][y, x] == gid, (case, gap, r["second_id"][y, x], gid)
            assert r["second_depth"][y, x] == pytest.approx(rng, rel=1e-6), (case, gap)
            assert r["has_second"][y, x] == (gid >= 0)
            # no ray sees another's Gaussians: what this pixel's alpha test lets through are its own, all of them
            p = y * W + x
            seen = np.sort(t["idx"][p][t["hit"][p]])
            assert (seen == members[case]).all(), (case, seen)
        if gap in s2.GAPS:
            for case, answers in ANSWERS.items():
                x, y = want[case][:2]
                assert r["second_depth"][y, x] == pytest.approx(answers[s2.GAPS.index(gap)], rel=1e-6), (case, gap)
    # where the walks have to go: the late wall's strongest return and the far second's wall sit in the second 64-entry chunk, and
    # the second walk reaches list position 64 of the far ray with best2 of about 0.002 in hand and T far above it
    want = s2.placed(W)[1]
    t = rs["table"]
    x, y = want["late wall"][:2]
    assert t["pos"][y * W + x] >= 64
    for gap in s2.GAPS:
        r = by_gap[gap]
        x, y = want["far second"][:2]
        p = y * W + x
        pos2 = int(r["pick"]["pos2"][p])
        assert pos2 >= 64 and int(t["pos"][p]) == 0
        best2 = np.where(r["pick"]["candidate"][p], t["weight"][p], 0.0)[:64].max()
        assert 0.0015 < best2 <= 0.0025 and t["T_after"][p][63] > 0.3      # (0.0025 from the layer at 10.01 m; 0.0019 from the one at 10.51 m)
    x, y = want["nothing"][:2]
    assert not rs["has_taker"][y, x]


@pytest.mark.parametrize("name", s2.SCENES)
def test_undecided_pixels_stay_under_the_cap(name, restated):
    """On every scene and gap the GPU tests use, at most CAP = 2 % of the pixels that have a taker are undecided -- a condition on the
    scenes, not a measurement; a pixel has a second return only where it has a taker, and then another Gaussian than the strongest."""
    _, W, rs, by_gap = restated[name]
    for gap, r in by_gap.items():
        frac = s2.undecided_fraction(r)
        print(f"{name} G={s2.gap_tag(gap)}: {int(r['has_taker'].sum())} pixels with a taker, {int(r['has_second'].sum())} with a second return, "
              f"undecided {frac:.4f} (strongest alone {sr.undecided_fraction(rs):.4f})")
        assert r["has_taker"].sum() >= 20 and frac <= s2.CAP
        assert not (r["has_second"] & ~r["has_taker"]).any()
        has = r["second_id"] >= 0
        assert (has == r["has_second"]).all() and (r["second_depth"][~has] == 0).all() and (r["second_depth"][has] > 0).all()
        assert (r["second_id"][has] != r["strongest_id"][has]).all()
        away = np.abs(r["second_depth"] - rs["strongest_depth"])[has]
        assert (away >= s2.gap_value(gap) - 1e-5).all()


def test_random_scenes_exercise_the_rule(restated):
    """On every random scene: pixels whose second return at G = 0.505 is another Gaussian than at G = 0 (the gap matters), pixels that
    lose their second return to the gap or have a single taker, and second returns deeper in the list than the strongest one."""
    for name in mr.RANDOM:
        by_gap = restated[name][3]
        r0, r1 = by_gap[None], by_gap[0.505]
        moved = r0["has_second"] & (r0["second_id"] != r1["second_id"])
        behind = r1["has_second"].ravel() & (r1["pick"]["pos2"] > r1["table"]["pos"])
        print(f"{name}: the gap changes the second return on {int(moved.sum())} pixels; behind the strongest on {int(behind.sum())}")
        assert moved.sum() >= 20 and behind.sum() >= 20, name
    assert any((restated[n][3][0.505]["has_taker"] & ~restated[n][3][0.505]["has_second"]).sum() >= 5 for n in s2.SCENES)


@pytest.mark.parametrize("name", s2.SCENES)
def test_nothing_behind_the_second_walks_exit_can_win(name, restated):
    """The kernel's second walk leaves a pixel at its first T <= best2 once best2 > 0.  On the float64 table: no candidate behind that
    position has a larger weight than the best candidate up to it (a later weight is alpha' T' <= 0.99 T), so the pick of the whole
    list is the pick up to the exit."""
    for gap, r in restated[name][3].items():
        first, behind, best2, pos2 = s2.exit_positions(r)
        if first.size:
            print(f"{name} G={s2.gap_tag(gap)}: mean exit position of the second walk {1 + first.mean():.1f}")
        assert (behind <= best2).all() and (pos2 <= first).all()


PROBE = r"""
#include <stdio.h>
#include <string.h>
#include "switches.h"
int main() {
    const float g = lg::return_gap();
    unsigned bits;
    memcpy(&bits, &g, 4);
    printf("%d%d%d%d %08x\n", lg::median_depth_requested() ? 1 : 0, lg::strongest_depth_requested() ? 1 : 0, lg::second_depth_requested() ? 1 : 0,
           lg::picked_depth_requested() ? 1 : 0, bits);
    return 0;
}
"""
# value of LIDARGS_DEPTH: (median, strongest, second, picked) as the probe prints them, depth_mode()
DEPTH_CASES = {None: ("0000", "expected"), "": ("0000", "expected"), "second": ("0011", "second"), "Second": ("0000", "expected"),
               "second ": ("0000", "expected"), "2": ("0000", "expected"), "median": ("1001", "median"), "strongest": ("0101", "strongest"),
               "seconds": ("0000", "expected"), "secon": ("0000", "expected")}
FLT_MAX = "340282346638528859811704183484516925440"
FIRST_INFINITE = "340282356779733661637539395458142568448"       # 2^128 - 2^103: from here on the nearest float32 is infinity
# value of LIDARGS_RETURN_GAP: the gap in metres (as a float32)
GAP_CASES = {None: 0.0, "": 0.0, "0": 0.0, "0.505": 0.505, ".5": 0.5, "2.": 2.0, "1e0": 0.0, "-1": 0.0, "+1": 0.0, "0.5 ": 0.0, " 0.5": 0.0,
             "nan": 0.0, "inf": 0.0, "1,5": 0.0, "7" * 400: 0.0, ".": 0.0, "0x10": 0.0, "1_0": 0.0, "007.250": 7.25, "1.5.2": 0.0,
             "0." + "0" * 400 + "1": 0.0, FLT_MAX: 3.4028234663852886e38, FIRST_INFINITE: 0.0, FLT_MAX + ".5": 3.4028234663852886e38}


def _bits(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", np.float32(x)))[0]


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    """The probe, plain and with the address and undefined-behaviour sanitizers: host code in a program of its own, their runtimes
    linked statically (as tests/test_switches_cpu.py builds its probe)."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("second_probe")
    (d / "probe.cpp").write_text(PROBE)
    built = {}
    sanitize = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    for name, flags in (("plain", ["-O1"]), ("sanitized", ["-O1"] + sanitize)):
        exe = str(d / name)
        subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, str(d / "probe.cpp"), "-o", exe], check=True)
        built[name] = exe
    return built


def _probe(exe, depth, gap):
    env = {k: v for k, v in os.environ.items() if k not in ("LIDARGS_DEPTH", "LIDARGS_RETURN_GAP")}
    if depth is not None:
        env["LIDARGS_DEPTH"] = depth
    if gap is not None:
        env["LIDARGS_RETURN_GAP"] = gap
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (depth, gap, r.stderr[-3000:])
    return r.stdout.split()


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_switch_and_the_gap_parse_as_specified(build, probes, monkeypatch):
    """Only the literal `second` selects the mode (and sets picked); LIDARGS_RETURN_GAP is accepted iff the whole string matches
    [0-9]+(\\.[0-9]*)?|\\.[0-9]+ and is finite as a float32.  The header compiles as a plain C++ program under -Wall -Wextra -Werror;
    the Python package's depth_mode() and return_gap() give the same answers on the same cases, the gap bit for bit."""
    from diff_lidargs_rasterization import depth_mode, return_gap
    exe = probes[build]
    for value, (flags, mode) in DEPTH_CASES.items():
        assert _probe(exe, value, None) == [flags, "00000000"], value
        assert _probe(exe, value, "0.505")[0] == flags, value
        monkeypatch.delenv("LIDARGS_DEPTH", raising=False) if value is None else monkeypatch.setenv("LIDARGS_DEPTH", value)
        assert depth_mode() == mode, value
    monkeypatch.delenv("LIDARGS_DEPTH", raising=False)
    for value, gap in GAP_CASES.items():
        for depth in ("second", None):                                    # (the parse does not depend on the mode; its use does)
            flags, bits = _probe(exe, depth, value)
            assert bits == _bits(gap), (value, bits, gap)
            assert flags == ("0011" if depth else "0000")
        monkeypatch.delenv("LIDARGS_RETURN_GAP", raising=False) if value is None else monkeypatch.setenv("LIDARGS_RETURN_GAP", value)
        got = return_gap()
        assert isinstance(got, float) and _bits(got) == _bits(gap) and got == float(np.float32(gap)), (value, got, gap)
