"""LIDARGS_DEPTH=strongest on the GPU: the strongest-return range of the 3-D rasterizer, forward and backward (DESIGN.md "Median-range
depth", the strongest-return rule).

Reference: tests/strongest_ref.py -- the rule restated on the CPU oracle's forward state, and the float64 autograd of a forward whose
depth is depth[strongest_id] (depth_modes.reference).  A pixel whose decision sits within rounding of a threshold or whose two largest
weights are within 1e-3 of each other is undecided (strongest_ref.py says when): it gives no vote in the forward and gets a zero
upstream depth gradient; tests/test_strongest_depth_cpu.py holds every scene used here to at most 2 % of them.

Scenes (strongest_ref.SCENES): those of the median tests and the hand-placed rays of strongest_ref.placed, 16 rows x 64 / 250 / 256
columns.  Built like tests/test_median_depth_gpu.py on the harness of tests/depth_modes.py: every scene runs in four child processes
-- LIDARGS_FUSED = 0 / 1 x LIDARGS_TILE_ROWS = 4 / 32 -- started together; a fifth child does what hangs on the buffers and the
refusals.  LIDARGS_DEPTH is read at every forward and is set inside the children only.
"""
import numpy as np
import pytest

import depth_modes as dm
import median_ref as mr
import strongest_ref as sr
from depth_modes import BUFFER_SCENE, H, IMAGE_KEYS, PLANS, REFUSING, same_bits
from util import hip_forward_backward, parity

pytestmark = pytest.mark.gpu

REJECTED = ("", "Strongest", "strongest ", "1", "expected")       # values of the switch that ask for the default mode


def child_plan(refs, out):
    """depth_modes.child_plan; the hand-placed rays under `median` as well."""
    def median_too(name, scene, W):
        return {f"{name}.median.depth": dm.with_env("median", None, lambda: hip_forward_backward(scene, W, H))["depth"]} if name in sr.PLACED else {}
    dm.child_plan(sr, "strongest", refs, out, also=median_too)


def child_buffers(refs, out):
    dm.child_buffers(sr, "strongest", REJECTED, ("median",), refs, out)


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """depth_modes.scene_refs: per scene the restatement, the float64 reference gradients and the CPU oracle's default-mode backward."""
    return dm.scene_refs(sr, tmp_path_factory.mktemp("strongest"))


@pytest.fixture(scope="module")
def runs(hip_lib_built, refs, tmp_path_factory):
    """{plan: arrays of child_plan} and {"buffers": arrays of child_buffers}, the five children running side by side, each under its
    own time limit."""
    return dm.start_children("test_strongest_depth_gpu", refs["path"], tmp_path_factory.mktemp("strongest_runs"))


@pytest.mark.parametrize("name", sr.SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_forward_returns_the_strongest_return(plan, name, runs, refs):
    """On every decided pixel the range of the restatement's Gaussian comes back (a wrong neighbour differs by metres, which no
    tolerance hides: every decided pixel is held to RTOL, none is excused), 0 where no pixel takes anything; colour, occupancy and
    radii are the same child's default forward, bit for bit; the scene's second strongest forward is the first, bit for bit."""
    r, ref = runs[plan], refs[name]["ref"]
    dm.check_decided_pixels_return_the_restatements_range(f"{plan}.{name}", r[f"{name}.strongest.depth"][0], ref, ref["strongest_depth"], ref["has_taker"])
    for k in ("color", "occ", "radii"):
        assert same_bits(r[f"{name}.strongest.{k}"], r[f"{name}.default.{k}"]), k
    for k in IMAGE_KEYS:
        assert same_bits(r[f"{name}.strongest.{k}"], r[f"{name}.strongest0.{k}"]), k
    # the default mode of the same child still returns the expected range
    parity(f"{plan}.{name}.expected depth", r[f"{name}.default.depth"][0], refs[name]["oracle0"]["depth"][0])


@pytest.mark.parametrize("W", [64, 250, 256])
@pytest.mark.parametrize("plan", list(PLANS))
def test_hand_placed_rays(plan, W, runs):
    """The rays whose answer is known by arithmetic.  Ten layers of opacity 0.1 in front of a wall of 0.9 at 20 m must return the wall:
    the same child's median forward returns the 7th layer (10.06 m) and its default forward a point in the air between them -- which
    is all `strongest`, an unknown value, gave before the mode existed (these assertions fail without the feature)."""
    r = runs[plan]
    got, median, default = (r[f"strongest{W}.{mode}.depth"][0] for mode in ("strongest", "median", "default"))
    want = sr.placed(W)[1]
    for case, (x, y, rng, _) in want.items():
        assert got[y, x] == pytest.approx(rng, rel=1e-5), (case, got[y, x], rng)
    x, y = want["veil"][:2]
    assert got[y, x] == pytest.approx(20.0, rel=1e-5)
    assert median[y, x] == pytest.approx(10.06, rel=1e-5)
    assert 10.5 < default[y, x] < 19.5
    for case, rng in (("late wall", 20.0), ("thin", 10.0), ("never", 10.0), ("0.4/0.9", 20.0), ("0.6/0.9", 10.0)):
        x, y = want[case][:2]
        assert got[y, x] == pytest.approx(rng, rel=1e-5), case
    x, y = want["nothing"][:2]
    assert got[y, x] == 0.0


@pytest.mark.parametrize("name", sr.BACKWARD_SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_backward_matches_the_float64_autograd_of_the_restatement(plan, name, runs, refs):
    """All six gradient arrays against torch.autograd of the float64 forward whose depth is depth[strongest_id], upstream depth gradients
    masked on undecided pixels: util.parity, default tolerances, on median_ref.BACKWARD_SCENES (whose float32 budget
    tests/test_median_depth_cpu.py asserts in the default mode)."""
    dm.check_backward_against_float64(f"{plan}.{name}", runs[plan], f"{name}.strongest", refs[name]["ref"], dm.miss_detail(runs[plan], name, refs[name]))


@pytest.mark.parametrize("name", sr.SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_without_a_depth_gradient_the_backward_is_the_default_modes(plan, name, runs, refs):
    """dL/ddepth = 0: the blend's depth terms and the add to the picked Gaussian both vanish, and the gradients are the default mode's
    on the same scene within the backward's own run-to-run band (float atomics in scheduling order)."""
    dm.check_no_depth_gradient_gives_the_default_backward(f"{plan}.{name}", runs[plan], f"{name}.strongest0", f"{name}.default0", refs[name]["oracle0_64"])


def test_depth_gradient_lands_on_exactly_one_gaussian(runs, refs):
    """strongest - strongest0 is the depth part alone: dL/dmeans3D rows differ exactly for the Gaussians that are some decided pixel's
    strongest return with a non-zero upstream gradient (one Gaussian per pixel), and colours / opacities carry none of it."""
    for plan in PLANS:
        for name in mr.RANDOM:
            dm.check_depth_gradient_lands_on_one_gaussian(f"{plan}.{name}", runs[plan], f"{name}.strongest", f"{name}.strongest0", refs[name]["ref"],
                                                          "strongest_id", refs[name]["oracle0_64"])


def test_buffer_sizes_and_values_of_the_switch(runs):
    """The buffers are a median forward's: only the image buffer grows, by the id plane (4 B per pixel, plus alignment); unset, empty
    and any value but the literal -- `Strongest` and a trailing blank among them -- ask for the default sizes, also after the mode has
    been used in the process."""
    b = runs["buffers"]
    like_default = dict({value: b[f"sizes[{value}]"] for value in REJECTED}, set_and_unset=b["sizes_set_and_unset"])
    dm.check_buffer_sizes(b["sizes_never_set"], b["sizes_switch_on"], (b["sizes_median"],), like_default, H * mr.RANDOM[BUFFER_SCENE][2])


def test_the_id_plane_names_the_restatements_gaussian(runs, refs):
    b, ref = runs["buffers"], refs[BUFFER_SCENE]["ref"]
    dm.check_id_plane("strongest", b["strongest_id"], ref, "strongest_id")
    assert (ref["strongest_id"] >= 0).sum() > 1000
    assert not same_bits(b["strongest.depth"], b["never_set.depth"])


def test_backward_twice_and_on_cloned_buffers_with_the_variable_unset(runs, refs):
    """The mode travels in the buffers: forward under the switch, variable removed, then backward, backward again and backward on clones
    of every saved tensor -- all the reference's gradients, and each other's within the run-to-run band."""
    dm.check_backward_twice_and_on_clones(runs["buffers"], refs[BUFFER_SCENE]["ref"])


def test_a_default_buffer_gets_the_default_gradients_after_a_strongest_forward(runs, refs):
    """The buffer's mode bit decides, not the process (depth_modes.check_default_buffer_after_a_picked_forward)."""
    up = np.load(refs["path"])
    grads = (up[f"{BUFFER_SCENE}.gc"], up[f"{BUFFER_SCENE}.gd_masked"], up[f"{BUFFER_SCENE}.go"])
    dm.check_default_buffer_after_a_picked_forward(runs["buffers"], refs[BUFFER_SCENE]["scene"], refs[BUFFER_SCENE]["W"], grads)


@pytest.mark.parametrize("case", list(REFUSING))
def test_entry_points_the_mode_does_not_cover_refuse_it(case, runs):
    """The surfel variant, shells and wedges, the enqueue-only forward, and lidargs_forward under LIDARGS_DETERMINISTIC=1 as well: a
    RuntimeError naming the variable and the entry point.  Without the switch they run, before and after."""
    dm.check_refusal(case, runs["buffers"])
