"""LIDARGS_DEPTH=median without a GPU: the restatement (tests/median_ref.py) on rays whose answer is known by arithmetic, the cap on
undecided pixels for every scene the GPU tests use, and the switch's parse rule through the probe around csrc/switches.h (tests/depth_modes.py)."""
import numpy as np
import pytest

import depth_modes as dm
import median_ref as mr
from oracle import lgo


@pytest.fixture(scope="module")
def restated():
    """{scene: (scene, W, oracle forward, restatement)}, once for the module."""
    out = {}
    for name in mr.SCENES:
        scene, W = mr.scene(name)
        f = dm.oracle_forward(scene, W)
        out[name] = (scene, W, f, mr.restate(f, scene, W, mr.H))
    return out


@pytest.mark.parametrize("W", [64, 250, 256])
def test_hand_placed_rays(W, restated):
    """Two Gaussians on one ray at 10 m and 20 m: opacities 0.4 / 0.9 leave T = 0.6 behind the first, so the second is the median (the
    expected range is 10 x 0.4 + 20 x 0.9 x 0.6 = 14.8, a point no surface is at); 0.6 / 0.9 cross at the first.  One opaque Gaussian
    gives its range, a ray without a taker 0 and no id, two of opacity 0.2 never reach one half (the last taker), 300 of opacity 0.02
    cross at the 35th (0.98^34 = 0.503, 0.98^35 = 0.493)."""
    scene, _, f, r = restated[f"placed{W}"]
    want = mr.placed(W)[1]
    for case, (x, y, rng, gid) in want.items():
        assert r["decided"][y, x], case
        assert r["median_id"][y, x] == gid, (case, r["median_id"][y, x], gid)
        assert r["median_depth"][y, x] == pytest.approx(rng, rel=1e-6), case
    x, y = want["0.4/0.9"][:2]
    assert r["median_depth"][y, x] == pytest.approx(20.0, rel=1e-6)
    assert f.depth[0][y, x] == pytest.approx(14.8, rel=5e-3) and r["expected"][y, x] == pytest.approx(float(f.depth[0][y, x]), rel=1e-5)
    x, y = want["0.6/0.9"][:2]
    assert r["median_depth"][y, x] == pytest.approx(10.0, rel=1e-6)
    x, y = want["thin"][:2]
    assert r["n_takers_to_median"][y, x] == 35 and r["crossed"][y, x]
    x, y = want["never"][:2]
    assert not r["crossed"][y, x] and r["median_depth"][y, x] == pytest.approx(20.0, rel=1e-6)
    x, y = want["nothing"][:2]
    assert not r["has_taker"][y, x] and r["median_depth"][y, x] == 0.0 and r["median_id"][y, x] == -1


@pytest.mark.parametrize("name", mr.SCENES)
def test_restated_blend_is_the_oracles_and_undecided_pixels_stay_under_the_cap(name, restated):
    """The restatement takes the entries the oracle takes (its colour, expected range and occupancy are the oracle's images), and on every
    scene the GPU tests use at most CAP = 2 % of the pixels that have a taker are undecided -- a condition on the scenes, not a measurement."""
    scene, W, f, r = restated[name]
    np.testing.assert_allclose(r["color"], f.color, rtol=0, atol=3e-5)
    np.testing.assert_allclose(r["expected"], f.depth[0], rtol=3e-5, atol=3e-4)
    np.testing.assert_allclose(r["occ"], f.occ[0], rtol=0, atol=3e-5)
    frac = dm.undecided_fraction(r)
    print(f"{name}: {int(r['has_taker'].sum())} pixels with a taker, {int(r['crossed'].sum())} cross one half, undecided {frac:.4f}")
    assert r["has_taker"].sum() >= 20 and frac <= mr.CAP
    # a median is a taker in front of the crossing: its range is never behind the expected range's farthest contributor
    has = r["median_id"] >= 0
    assert (has == r["has_taker"]).all() and (r["median_depth"][~has] == 0).all() and (r["median_depth"][has] > 0).all()


def test_random_scenes_exercise_the_rule(restated):
    """Lists longer than one 64-entry chunk, rays that cross and rays that do not, pixels without a taker, and pixels where the median
    and the expected range differ by metres."""
    for name in mr.RANDOM:
        scene, W, f, r = restated[name]
        assert r["crossed"].sum() >= 50 and (r["has_taker"] & ~r["crossed"]).sum() >= 10, name
        assert (np.abs(r["median_depth"] - r["expected"])[r["has_taker"]] > 1.0).sum() >= 20, name
    assert any((~restated[n][3]["has_taker"]).sum() >= 10 for n in mr.RANDOM)
    assert any(dm.pixel_lists(restated[n][2], restated[n][1], mr.H)[1].sum(1).max() > 64 for n in mr.RANDOM)


def _conforming_evaluations(scene, W, grads):
    """The CPU oracle's forward + backward as it is, with every cos / sin / atan2 / tan / exp result moved inside its error bound
    (util.ULP_MODES, as util.oracle_envelope does) and with the backward's pixels visited in reverse order: (name, result) pairs."""
    import ctypes as C
    from util import ULP_MODES, oracle_forward_backward
    L = lgo.lib()
    yield "plain", oracle_forward_backward(scene, W, mr.H, grads)
    for mode, seed in ULP_MODES:
        L.lgo_set_ulp_perturbation(C.c_int(mode), C.c_uint(seed))
        try:
            r = oracle_forward_backward(scene, W, mr.H, grads)
        finally:
            L.lgo_set_ulp_perturbation(C.c_int(0), C.c_uint(0))
        yield f"ulp {mode}/{seed}", r
    L.lgo_set_reverse_pixel_order(C.c_int(1))
    try:
        r = oracle_forward_backward(scene, W, mr.H, grads)
    finally:
        L.lgo_set_reverse_pixel_order(C.c_int(0))
    yield "reverse order", r


def _evaluations_over_the_budget(name, restated):
    """-> [(evaluation, array, message)] for every conforming float32 evaluation of the reference that misses util.parity's default
    budget against the float64 chain of the restatement, without a depth gradient (nothing of the median mode is involved)."""
    from util import GRAD_KEYS_SR, PARITY_LOG, parity
    scene, W, f, _ = restated[name]
    gc, gd, go = mr.upstream(name)
    nodepth = (gc, np.zeros_like(gd), go)
    ref = dm.reference(scene, W, mr.H, nodepth, mr.RULE, f=f)
    missed = []
    for what, r in _conforming_evaluations(scene, W, nodepth):
        for k in GRAD_KEYS_SR:
            try:
                parity(f"oracle[{what}].{name}.{k}", r[k], ref[k], verbose=False)
            except AssertionError as e:
                missed.append((what, k, str(e)))
                if PARITY_LOG and PARITY_LOG[-1]["name"] == f"oracle[{what}].{name}.{k}":
                    PARITY_LOG.pop()                                  # (the oracle against itself: not part of the suite's budget report)
    return missed


@pytest.mark.parametrize("name", mr.BACKWARD_SCENES)
def test_float32_can_meet_the_gradient_budget_on_the_backward_scenes(name, restated):
    """The condition on median_ref.BACKWARD_SCENES: every conforming float32 evaluation of the reference meets util.parity's default
    budget against the float64 chain of the restatement, on all six arrays."""
    missed = _evaluations_over_the_budget(name, restated)
    assert not missed, missed


@pytest.mark.parametrize("name", [n for n in mr.SCENES if n not in mr.BACKWARD_SCENES])
def test_the_other_scenes_do_not_qualify(name, restated):
    """... and BACKWARD_SCENES leaves out no scene that meets it: on each of the others some conforming evaluation of the reference
    itself misses the budget."""
    missed = _evaluations_over_the_budget(name, restated)
    print(name, missed)
    assert missed


def test_reference_gradient_of_the_depth_lands_on_the_median_gaussian(restated):
    """The float64 reference: with only dL/ddepth upstream, a Gaussian has a gradient exactly where it is some decided pixel's median,
    and dL/dmeans3D is dL/ddepth x the unit ray to the mean (depth = |view-space mean|), summed over its pixels."""
    name = "shell64"
    scene, W, f, r = restated[name]
    rng = np.random.default_rng(5)
    gd = rng.normal(size=(1, mr.H, W)).astype(np.float32)
    ref = dm.reference(scene, W, mr.H, (np.zeros((2, mr.H, W), np.float32), gd, np.zeros((1, mr.H, W), np.float32)), mr.RULE, f=f)
    P = scene["means3D"].shape[0]
    want = np.zeros(P)
    ok = r["decided"] & (r["median_id"] >= 0)
    np.add.at(want, r["median_id"][ok], gd[0][ok].astype(np.float64))
    V = np.asarray(scene["viewmatrix"], np.float64).reshape(4, 4)
    pv = scene["means3D"].astype(np.float64) @ V[:3, :3] + V[3, :3]
    unit = pv / np.linalg.norm(pv, axis=1, keepdims=True)
    np.testing.assert_allclose(ref["dL_dmeans3D"], (want[:, None] * unit) @ V[:3, :3].T, rtol=1e-9, atol=1e-12)
    for k in ("dL_dcolors", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dmeans2D"):
        assert np.abs(ref[k]).max() == 0.0, k


@pytest.mark.parametrize("value", [None, "", "median", "Median", "1", "median ", "expected"],
                         ids=["unset", "empty", "median", "Median", "1", "trailing blank", "expected"])
def test_the_switch_parses_as_specified(value, tmp_path_factory):
    """Only the literal `median` turns the mode on; the header compiles as a plain C++ program under -Wall -Wextra -Werror."""
    exe = dm.build_probe(tmp_path_factory)
    if not exe:
        pytest.skip("no g++")
    assert dm.DEPTH_CASES[value] == ("median" if value == "median" else "expected")
    assert dm.probe(exe, value, None)[0] == dm.DEPTH_CASES[value], value


def test_depth_mode_of_the_python_package(monkeypatch):
    """diff_lidargs_rasterization.depth_mode() reads the same variable by the same rule."""
    from diff_lidargs_rasterization import depth_mode
    for value, want in ((None, "expected"), ("", "expected"), ("median", "median"), ("Median", "expected"), ("1", "expected")):
        if value is None:
            monkeypatch.delenv("LIDARGS_DEPTH", raising=False)
        else:
            monkeypatch.setenv("LIDARGS_DEPTH", value)
        assert depth_mode() == want, value
