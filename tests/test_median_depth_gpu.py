"""LIDARGS_DEPTH=median on the GPU: the median range of the 3-D rasterizer, forward and backward (DESIGN.md "Median-range depth").

Reference: tests/median_ref.py -- the rule restated on the CPU oracle's forward state, and the float64 autograd of a forward whose depth
is depth[median_id] (depth_modes.reference).  A pixel whose decision sits within rounding of a threshold is undecided (median_ref.py
says when): it gives no vote in the forward and gets a zero upstream depth gradient; tests/test_median_depth_cpu.py holds every scene
used here to at most 2 % of them.

Scenes (median_ref.SCENES): four random ones and the hand-placed rays, 16 rows x 64 / 250 / 256 columns (250: a ragged last tile
column; the first column's Gaussians reach over the seam), lists of more than one 64-entry chunk, rays that cross one half, rays that
never do and pixels without a taker.  Every scene runs in four child processes -- LIDARGS_FUSED = 0 / 1 (the median launch sits behind
either form of the blend) x LIDARGS_TILE_ROWS = 4 / 32, which are read once per process -- started together; a fifth child does what
hangs on the buffers and the refusals (tests/depth_modes.py has the harness and the bodies of the tests every picked mode shares).
LIDARGS_DEPTH itself is read at every forward and is set inside the children only.
"""
import numpy as np
import pytest

import depth_modes as dm
import median_ref as mr
from depth_modes import BUFFER_SCENE, H, PLANS, REFUSING, same_bits
from util import parity

pytestmark = pytest.mark.gpu

REJECTED = ("", "Median", "1", "expected")       # values of the switch that ask for the default mode


def child_plan(refs, out):
    dm.child_plan(mr, "median", refs, out)


def child_buffers(refs, out):
    dm.child_buffers(mr, "median", REJECTED, (), refs, out)


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """depth_modes.scene_refs: per scene the restatement, the float64 reference gradients and the CPU oracle's default-mode backward."""
    return dm.scene_refs(mr, tmp_path_factory.mktemp("median"))


@pytest.fixture(scope="module")
def runs(hip_lib_built, refs, tmp_path_factory):
    """{plan: arrays of child_plan} and {"buffers": arrays of child_buffers}, the five children running side by side."""
    return dm.start_children("test_median_depth_gpu", refs["path"], tmp_path_factory.mktemp("median_runs"))


@pytest.mark.parametrize("name", mr.SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_forward_returns_the_median_range(plan, name, runs, refs):
    """On every decided pixel the range of the restatement's Gaussian comes back (a wrong neighbour differs by metres, which no
    tolerance hides: every decided pixel is held to the parity metric's bar, none is a `flip`), 0 where no pixel takes anything;
    colour, occupancy and radii are the same child's default forward, bit for bit."""
    r, ref = runs[plan], refs[name]["ref"]
    got, dec, want = r[f"{name}.median.depth"][0], ref["decided"], ref["median_depth"]
    st = parity(f"{plan}.{name}.median depth", got[dec], want[dec])
    dm.check_decided_pixels_return_the_restatements_range(f"{plan}.{name}", got, ref, want, ref["has_taker"])
    for k in ("color", "occ", "radii"):
        assert same_bits(r[f"{name}.median.{k}"], r[f"{name}.default.{k}"]), k
    # the default mode of the same child still returns the expected range
    parity(f"{plan}.{name}.expected depth", r[f"{name}.default.depth"][0], refs[name]["oracle0"]["depth"][0])
    assert st["n"] > 0


@pytest.mark.parametrize("W", [64, 250, 256])
@pytest.mark.parametrize("plan", list(PLANS))
def test_hand_placed_rays(plan, W, runs):
    """The rays whose answer is known by arithmetic.  Opacities 0.4 / 0.9 at 10 m / 20 m must return 20 m -- the expected range, which is
    all the library returned before the mode existed, is 14.8 m there (this assertion fails without the feature)."""
    r = runs[plan]
    got, default = r[f"placed{W}.median.depth"][0], r[f"placed{W}.default.depth"][0]
    for case, (x, y, rng, _) in mr.placed(W)[1].items():
        assert got[y, x] == pytest.approx(rng, rel=1e-5), (case, got[y, x], rng)
    x, y = mr.placed(W)[1]["0.4/0.9"][:2]
    assert got[y, x] == pytest.approx(20.0, rel=1e-5)
    assert default[y, x] == pytest.approx(14.8, rel=5e-3)
    x, y = mr.placed(W)[1]["nothing"][:2]
    assert got[y, x] == 0.0


@pytest.mark.parametrize("name", mr.BACKWARD_SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_backward_matches_the_float64_autograd_of_the_restatement(plan, name, runs, refs):
    """All six gradient arrays against torch.autograd of the float64 forward whose depth is depth[median_id], upstream depth gradients
    masked on undecided pixels: util.parity, default tolerances.  On the scenes where every conforming float32 evaluation of the
    reference itself meets that budget (median_ref.BACKWARD_SCENES says which, and why; tests/test_median_depth_cpu.py asserts it)."""
    dm.check_backward_against_float64(f"{plan}.{name}", runs[plan], f"{name}.median", refs[name]["ref"], dm.miss_detail(runs[plan], name, refs[name]))


@pytest.mark.parametrize("name", mr.SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_without_a_depth_gradient_the_backward_is_the_default_modes(plan, name, runs, refs):
    """dL/ddepth = 0: the blend's depth terms and the median add both vanish, and the gradients are the default mode's on the same scene
    within the backward's own run-to-run band (float atomics in scheduling order)."""
    dm.check_no_depth_gradient_gives_the_default_backward(f"{plan}.{name}", runs[plan], f"{name}.median0", f"{name}.default0", refs[name]["oracle0_64"])


def test_depth_gradient_lands_on_exactly_one_gaussian(runs, refs):
    """median - median0 is the depth part alone: dL/dmeans3D rows differ exactly for the Gaussians that are some decided pixel's median
    with a non-zero upstream gradient (one Gaussian per pixel), and colours / opacities carry none of it."""
    for plan in PLANS:
        for name in mr.RANDOM:
            dm.check_depth_gradient_lands_on_one_gaussian(f"{plan}.{name}", runs[plan], f"{name}.median", f"{name}.median0", refs[name]["ref"],
                                                          "median_id", refs[name]["oracle0_64"])


def test_buffer_sizes_and_values_of_the_switch(runs):
    """Only the image buffer grows, by the id plane (4 B per pixel, plus alignment); unset, empty and any value but the literal `median`
    ask for today's sizes -- also after the mode has been used in the process."""
    b = runs["buffers"]
    like_default = dict({value: b[f"sizes[{value}]"] for value in REJECTED}, set_and_unset=b["sizes_set_and_unset"])
    dm.check_buffer_sizes(b["sizes_never_set"], b["sizes_switch_on"], (), like_default, H * mr.RANDOM[BUFFER_SCENE][2])


def test_the_id_plane_names_the_restatements_gaussian(runs, refs):
    b, ref = runs["buffers"], refs[BUFFER_SCENE]["ref"]
    dm.check_id_plane("median", b["median_id"], ref, "median_id")
    assert (ref["median_id"] >= 0).sum() > 1000
    assert not same_bits(b["median.depth"], b["never_set.depth"])


def test_backward_twice_and_on_cloned_buffers_with_the_variable_unset(runs, refs):
    """The mode travels in the buffers: forward under the switch, variable removed, then backward, backward again (retain_graph) and
    backward on clones of every saved tensor -- all three the reference's gradients, and each other's within the run-to-run band."""
    dm.check_backward_twice_and_on_clones(runs["buffers"], refs[BUFFER_SCENE]["ref"])


def test_a_default_buffer_gets_the_default_gradients_after_a_median_forward(runs, refs):
    """The buffer's mode bit decides, not the process (depth_modes.check_default_buffer_after_a_picked_forward)."""
    up = np.load(refs["path"])
    grads = (up[f"{BUFFER_SCENE}.gc"], up[f"{BUFFER_SCENE}.gd_masked"], up[f"{BUFFER_SCENE}.go"])
    dm.check_default_buffer_after_a_picked_forward(runs["buffers"], refs[BUFFER_SCENE]["scene"], refs[BUFFER_SCENE]["W"], grads)


@pytest.mark.parametrize("case", list(REFUSING))
def test_entry_points_the_mode_does_not_cover_refuse_it(case, runs):
    """The surfel variant (it has a median plane of its own), shells and wedges, the enqueue-only forward, and lidargs_forward under
    LIDARGS_DETERMINISTIC=1 as well: a RuntimeError naming the variable and the entry point.  Without the switch they run, before and after."""
    dm.check_refusal(case, runs["buffers"])
