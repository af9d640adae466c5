"""LIDARGS_DEPTH=second without a GPU: the restatement (tests/second_ref.py) on rays whose answer is known by arithmetic, the cap on
undecided pixels for every scene and gap the GPU tests use, the bound the second walk's early exit rests on, and the parse rules of the
switch and of LIDARGS_RETURN_GAP through the probe around csrc/switches.h (tests/depth_modes.py), plain and under the sanitizers, held
against the Python package's depth_mode() and return_gap() on one case list."""
import numpy as np
import pytest

import depth_modes as dm
import median_ref as mr
import second_ref as s2
import strongest_ref as sr
from second_ref import ANSWERS


@pytest.fixture(scope="module")
def restated():
    """{scene: (scene, W, strongest restatement, {gap: second restatement})}, once for the module."""
    out = {}
    for name in s2.SCENES:
        scene, W = s2.scene(name)
        f = dm.oracle_forward(scene, W)
        rs = sr.restate(f, scene, W, s2.H)
        out[name] = (scene, W, rs, {gap: s2.restate(f, rs, gap) for gap in s2.gaps(name)})
    return out


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
        frac = dm.undecided_fraction(r)
        print(f"{name} G={s2.gap_tag(gap)}: {int(r['has_taker'].sum())} pixels with a taker, {int(r['has_second'].sum())} with a second return, "
              f"undecided {frac:.4f} (strongest alone {dm.undecided_fraction(rs):.4f})")
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


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_switch_and_the_gap_parse_as_specified(build, tmp_path_factory, monkeypatch):
    """Only the literal names select a mode -- `second` this one -- (picked: the mode is not `expected`); LIDARGS_RETURN_GAP is accepted
    iff the whole string matches [0-9]+(\\.[0-9]*)?|\\.[0-9]+ and is finite as a float32.  The header compiles as a plain C++ program
    under -Wall -Wextra -Werror; the Python package's depth_mode() and return_gap() give the same answers on the same cases, the gap
    bit for bit.  The cases are those of all three modes' tests (depth_modes.DEPTH_CASES, GAP_CASES)."""
    from diff_lidargs_rasterization import depth_mode, return_gap
    exe = dm.build_probe(tmp_path_factory, build)
    if not exe:
        pytest.skip("no g++")
    assert dm.DEPTH_CASES["second"] == "second" and all(dm.DEPTH_CASES[v] == "expected" for v in ("Second", "second ", "2", "seconds", "secon"))
    for value, mode in dm.DEPTH_CASES.items():
        assert mode == (value if value in ("median", "strongest", "second") else "expected")
        assert dm.probe(exe, value, None) == [mode, "00000000"], value
        assert dm.probe(exe, value, "0.505")[0] == mode, value
        monkeypatch.delenv(dm.SWITCH, raising=False) if value is None else monkeypatch.setenv(dm.SWITCH, value)
        assert depth_mode() == mode, value
    monkeypatch.delenv(dm.SWITCH, raising=False)
    for value, gap in dm.GAP_CASES.items():
        for depth in ("second", None):                                    # (the parse does not depend on the mode; its use does)
            mode, bits = dm.probe(exe, depth, value)
            assert bits == dm.float32_bits(gap), (value, bits, gap)
            assert mode == (depth or "expected")
        monkeypatch.delenv(dm.GAP, raising=False) if value is None else monkeypatch.setenv(dm.GAP, value)
        got = return_gap()
        assert isinstance(got, float) and dm.float32_bits(got) == dm.float32_bits(gap) and got == float(np.float32(gap)), (value, got, gap)
