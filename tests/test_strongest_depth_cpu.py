"""LIDARGS_DEPTH=strongest without a GPU: the restatement (tests/strongest_ref.py) on rays whose answer is known by arithmetic, the cap
on undecided pixels for every scene the GPU tests use, the bound the kernel's early exit rests on, and the switch's parse rule through the
probe around csrc/switches.h (tests/depth_modes.py)."""
import numpy as np
import pytest

import depth_modes as dm
import median_ref as mr
import strongest_ref as sr


@pytest.fixture(scope="module")
def restated():
    """{scene: (scene, W, oracle forward, strongest restatement, median restatement)}, once for the module."""
    out = {}
    for name in sr.SCENES:
        scene, W = sr.scene(name)
        f = dm.oracle_forward(scene, W)
        out[name] = (scene, W, f, sr.restate(f, scene, W, sr.H), mr.restate(f, scene, W, sr.H))
    return out


@pytest.mark.parametrize("W", [64, 250, 256])
def test_hand_placed_rays(W, restated):
    """The rays of strongest_ref.placed: 0.4 / 0.9 at 10 m / 20 m have weights 0.40 and 0.9 x 0.6 = 0.54 (the second), 0.6 / 0.9 have
    0.60 and 0.36 (the first), 0.2 / 0.2 have 0.20 and 0.16 (the first; the median mode returns its last taker, 20 m), 300 of opacity
    0.02 fall from the first on (the median is the 35th), ten layers of 0.1 in front of a wall stay at or under 0.10 against the wall's
    0.31 (the median is the 7th layer), and 100 layers of 0.005 leave T = 0.61 for the wall at list position 101."""
    scene, _, f, r, m = restated[f"strongest{W}"]
    _, want, members = sr.placed(W)
    t = r["table"]
    for case, (x, y, rng, gid) in want.items():
        assert r["decided"][y, x], case
        assert r["strongest_id"][y, x] == gid, (case, r["strongest_id"][y, x], gid)
        assert r["strongest_depth"][y, x] == pytest.approx(rng, rel=1e-6), case
        # no ray sees another's Gaussians: what this pixel's alpha test lets through are its own, all of them
        p = y * W + x
        seen = np.sort(t["idx"][p][t["hit"][p]])
        assert (seen == members[case]).all(), (case, seen)
    depth = lambda case, plane: float(plane[want[case][1], want[case][0]])
    for case, rng in (("0.4/0.9", 20.0), ("0.6/0.9", 10.0), ("never", 10.0), ("thin", 10.0), ("veil", 20.0), ("late wall", 20.0),
                      ("last column", 20.0), ("first column", 18.0)):
        assert depth(case, r["strongest_depth"]) == pytest.approx(rng, rel=1e-6), case
    # where the other two answers are: the median mode's, and the expected range
    assert depth("never", m["median_depth"]) == pytest.approx(20.0, rel=1e-6)
    assert depth("thin", m["median_depth"]) == pytest.approx(10.34, rel=1e-6)
    assert depth("veil", m["median_depth"]) == pytest.approx(10.06, rel=1e-6)
    assert 10.5 < depth("veil", f.depth[0]) < 19.5
    x, y = want["veil"][:2]
    assert r["top_weight"][y, x] == pytest.approx(0.31, abs=0.01) and r["runner_up"][y, x] <= 0.10
    x, y = want["late wall"][:2]
    p = y * W + x
    pos = int(t["pos"][p])
    assert t["taken"][p][:pos].sum() == sr.LATE_N and pos >= 64               # the winner sits in the second 64-entry chunk ...
    assert t["T_after"][p][pos - 1] == pytest.approx(0.61, abs=0.01)          # ... with T = 0.61 in front of it
    assert (t["T_after"][p][:pos] > np.maximum.accumulate(t["weight"][p])[:pos]).all()   # so the exit must not fire before it
    x, y = want["nothing"][:2]
    assert not r["has_taker"][y, x] and r["strongest_depth"][y, x] == 0.0 and r["strongest_id"][y, x] == -1


@pytest.mark.parametrize("name", sr.SCENES)
def test_restated_blend_is_the_oracles_and_undecided_pixels_stay_under_the_cap(name, restated):
    """The restatement takes the entries the oracle takes (its colour, expected range and occupancy are the oracle's images), and on every
    scene the GPU tests use at most CAP = 2 % of the pixels that have a taker are undecided -- a condition on the scenes, not a measurement."""
    scene, W, f, r, _ = restated[name]
    np.testing.assert_allclose(r["color"], f.color, rtol=0, atol=3e-5)
    np.testing.assert_allclose(r["expected"], f.depth[0], rtol=3e-5, atol=3e-4)
    np.testing.assert_allclose(r["occ"], f.occ[0], rtol=0, atol=3e-5)
    frac = dm.undecided_fraction(r)
    print(f"{name}: {int(r['has_taker'].sum())} pixels with a taker, undecided {frac:.4f}")
    assert r["has_taker"].sum() >= 20 and frac <= sr.CAP
    has = r["strongest_id"] >= 0
    assert (has == r["has_taker"]).all() and (r["strongest_depth"][~has] == 0).all() and (r["strongest_depth"][has] > 0).all()


def test_random_scenes_exercise_the_rule(restated):
    """On every random scene at least 20 pixels where the strongest return and the median lie more than a metre apart; lists longer
    than one 64-entry chunk; pixels without a taker."""
    for name in mr.RANDOM:
        scene, W, f, r, m = restated[name]
        has = r["has_taker"]
        other = (r["strongest_id"] != m["median_id"]) & has
        far = (np.abs(r["strongest_depth"] - m["median_depth"]) > 1.0) & has
        print(f"{name}: strongest is not the median Gaussian on {other.sum() / has.sum():.2f} of the pixels with a taker, over 1 m away on "
              f"{far.sum() / has.sum():.2f}")
        assert far.sum() >= 20, name
    assert any((~restated[n][3]["has_taker"]).sum() >= 10 for n in mr.RANDOM)
    assert any(restated[n][3]["table"]["valid"].sum(1).max() > 64 for n in mr.RANDOM)


@pytest.mark.parametrize("name", sr.SCENES)
def test_nothing_behind_the_exit_can_win(name, restated):
    """The kernel's pixel leaves at its first T <= best.  On the float64 table: no entry behind that position has a larger weight than
    the best up to it (a later weight is alpha' T' <= 0.99 T)."""
    t = restated[name][3]["table"]
    first, behind, best = sr.exit_positions(t)
    lengths = t["valid"].sum(1)[t["taken"].any(1)]
    print(f"{name}: mean exit position {1 + first.mean():.1f} entries of a mean list of {lengths.mean():.1f}")
    assert (behind <= best).all()
    # ... and the pick of the whole list is the pick up to the exit
    rows = np.nonzero(t["taken"].any(1))[0]
    assert (t["pos"][rows] <= first).all()


@pytest.mark.parametrize("value", [None, "", "strongest", "median", "Strongest", "Median", "1", "strongest ", "expected"],
                         ids=["unset", "empty", "strongest", "median", "Strongest", "Median", "1", "trailing blank", "expected"])
def test_the_switch_parses_as_specified(value, tmp_path_factory):
    """Only the literals `strongest` and `median` select a mode; the header compiles as a plain C++ program under -Wall -Wextra -Werror."""
    exe = dm.build_probe(tmp_path_factory)
    if not exe:
        pytest.skip("no g++")
    assert dm.DEPTH_CASES[value] == (value if value in ("strongest", "median") else "expected")
    assert dm.probe(exe, value, None)[0] == dm.DEPTH_CASES[value], value


def test_depth_mode_of_the_python_package(monkeypatch):
    """diff_lidargs_rasterization.depth_mode() reads the same variable by the same rule."""
    from diff_lidargs_rasterization import depth_mode
    for value, want in ((None, "expected"), ("", "expected"), ("strongest", "strongest"), ("median", "median"), ("Strongest", "expected"),
                        ("strongest ", "expected"), ("1", "expected"), ("expected", "expected")):
        if value is None:
            monkeypatch.delenv("LIDARGS_DEPTH", raising=False)
        else:
            monkeypatch.setenv("LIDARGS_DEPTH", value)
        assert depth_mode() == want, value
