"""LIDARGS_DEPTH=second on the GPU: the second-return range of the 3-D rasterizer, forward and backward (the rule: csrc/switches.h
DepthMode::Second), with LIDARGS_RETURN_GAP unset and set.

Reference: tests/second_ref.py -- the rule restated on tests/strongest_ref.py's table of the CPU oracle's forward state, and the
float64 autograd of a forward whose depth is depth[second_id] (depth_modes.reference).  A pixel whose strongest return is undecided,
whose two heaviest candidates are within 1e-3 of each other or which has an entry within 1 mm of the gap's edge is undecided
(second_ref.py says when): it gives no vote in the forward and gets a zero upstream depth gradient; tests/test_second_depth_cpu.py
holds every scene and gap used here to at most 2 % of them.

Scenes (second_ref.SCENES): those of the strongest tests and the hand-placed rays of second_ref.placed, 16 rows x 64 / 250 / 256
columns, at the gap unset and 0.505 m (the hand-placed rays of this mode at 2.005 m as well).  Built like
tests/test_strongest_depth_gpu.py on the harness of tests/depth_modes.py: every scene runs in four child processes -- LIDARGS_FUSED =
0 / 1 x LIDARGS_TILE_ROWS = 4 / 32 -- started together; a fifth child does what hangs on the buffers and the refusals.  Both variables
are read at every forward and are set inside the children only.
"""
import os

import numpy as np
import pytest

import depth_modes as dm
import median_ref as mr
import second_ref as s2
import strongest_ref as sr
from depth_modes import BUFFER_SCENE, GAP, H, IMAGE_KEYS, PLANS, REFUSING, SWITCH, same_bits
from second_ref import ANSWERS
from util import GRAD_KEYS_SR, hip_forward_backward, oracle_backward_exact_sums, oracle_forward_backward

pytestmark = pytest.mark.gpu

BUFFER_GAP = 0.505
BACKWARD = [(name, 0.505) for name in s2.BACKWARD_SCENES] + [(s2.BACKWARD_UNSET, None)]      # (scene, gap) of the backward tests
BACKWARD_IDS = [f"{name}-G={s2.gap_tag(gap)}" for name, gap in BACKWARD]
REJECTED = ("Second", "second ", "2")            # values of the switch that ask for the default mode


def _key(name, gap):
    return f"{name}.second[{s2.gap_tag(gap)}]"


def child_plan(refs, out):
    """One child process: every scene's default forward and its `second` forward at every gap of the scene; for the (scene, gap) pairs
    of BACKWARD also the backward with the reference's masked depth gradient and with none, in both modes."""
    assert SWITCH not in os.environ and GAP not in os.environ
    up = np.load(refs)
    res = {}
    for name in s2.SCENES:
        scene, W = s2.scene(name)
        nodepth = (up[f"{name}.gc"], np.zeros((1, H, W), np.float32), up[f"{name}.go"])
        backward = name in s2.BACKWARD_SCENES
        r = dm.with_env(None, None, lambda: hip_forward_backward(scene, W, H, nodepth if backward else None))
        res.update({f"{name}.default0.{k}": r[k] for k in IMAGE_KEYS + (GRAD_KEYS_SR if backward else ())})
        for gap in s2.gaps(name):
            key = _key(name, gap)
            if (name, gap) in BACKWARD:
                masked = (nodepth[0], up[f"{key}.gd_masked"], nodepth[2])
                r = dm.with_env("second", gap, lambda: hip_forward_backward(scene, W, H, masked))
                res.update({f"{key}.{k}": r[k] for k in IMAGE_KEYS + GRAD_KEYS_SR})
                r = dm.with_env("second", gap, lambda: hip_forward_backward(scene, W, H, nodepth))
                res.update({f"{key}0.{k}": r[k] for k in IMAGE_KEYS + GRAD_KEYS_SR})
            else:
                r = dm.with_env("second", gap, lambda: hip_forward_backward(scene, W, H))
                res.update({f"{key}.{k}": r[k] for k in IMAGE_KEYS})
    np.savez(out, **res)
    print("OK")


def child_buffers(refs, out):
    """The fifth child: buffer sizes, the id planes of `strongest` and `second`, backward twice / on clones with both variables unset,
    a default forward's backward in a process that has made such buffers, the values of the switch, the gap without the mode, and the
    refusals."""
    assert SWITCH not in os.environ and GAP not in os.environ
    up = np.load(refs)
    name = BUFFER_SCENE
    fr = dm.Frame(*s2.scene(name), (up[f"{name}.gc"], up[f"{_key(name, BUFFER_GAP)}.gd_masked"], up[f"{name}.go"]))
    res = {}

    def record(tag, fwd, n_img, with_plane=True):
        res[f"{tag}.sizes"] = fr.sizes(fwd)
        res.update({f"{tag}.{k}": v for k, v in fr.images(fwd).items()})
        if with_plane:
            res[f"{tag}.id"] = fr.id_plane(fwd, n_img)

    plain = fr.forward()
    n_img = int(fr.sizes(plain)[2])
    record("never_set", plain, n_img, False)
    res.update({f"before.{k}": v for k, v in fr.backward(plain).items()})     # (no such forward yet in this process: the default launches)
    for value in REJECTED:
        res[f"sizes[{value}]"] = dm.with_env(value, None, lambda: fr.sizes(fr.forward()))
    record("gap_alone", dm.with_env(None, "0.505", fr.forward), n_img, False)         # LIDARGS_RETURN_GAP without the mode: nothing changes
    record("strongest_before", dm.with_env("strongest", None, fr.forward), n_img)
    record("strongest_with_gap", dm.with_env("strongest", "0.505", fr.forward), n_img)
    on = None
    for gap in s2.GAPS:
        fwd = dm.with_env("second", gap, fr.forward)
        record(f"second[{s2.gap_tag(gap)}]", fwd, n_img)
        if gap == BUFFER_GAP:
            on = fwd
    record("strongest_after", dm.with_env("strongest", None, fr.forward), n_img)
    res["sizes_median"] = dm.with_env("median", None, lambda: fr.sizes(fr.forward()))
    record("default_after", fr.backward_rounds(on, res), n_img, False)    # both variables are unset from here on: the mode travels in the buffers, the gap nowhere
    dm.refusals("second", "0.505", res, *s2.scene("shell64"))
    np.savez(out, **res)
    print("OK")


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """Per scene: the restatement at every gap of the scene; per (scene, gap) of BACKWARD the float64 reference gradients for upstream
    gradients whose depth part is masked on undecided pixels (depth_modes.reference), and per backward scene the CPU oracle's
    default-mode backward for the same upstream gradients without a depth part, with its exact sums.  Computed once; the upstream
    gradients go to the children in a file."""
    out, up = {}, {}
    for name in s2.SCENES:
        scene, W = s2.scene(name)
        gc, gd, go = s2.upstream(name)
        f = dm.oracle_forward(scene, W)
        rs = sr.restate(f, scene, W, H)
        entry = dict(scene=scene, W=W, strongest=rs, restated={gap: s2.restate(f, rs, gap) for gap in s2.gaps(name)}, ref={})
        up.update({f"{name}.gc": gc, f"{name}.go": go})
        if name in s2.BACKWARD_SCENES:
            nodepth = (gc, np.zeros_like(gd), go)
            entry["oracle0"] = oracle_forward_backward(scene, W, H, nodepth)
            entry["oracle0_64"] = oracle_backward_exact_sums(entry["oracle0"], nodepth)
        for gap in s2.gaps(name):
            if (name, gap) in BACKWARD:
                entry["ref"][gap] = dm.reference(scene, W, H, (gc, gd, go), s2.rule(gap), f=f)
                up[f"{_key(name, gap)}.gd_masked"] = entry["ref"][gap]["dL_ddepth_masked"]
        out[name] = entry
    path = str(tmp_path_factory.mktemp("second") / "upstream.npz")
    np.savez(path, **up)
    out["path"] = path
    return out


@pytest.fixture(scope="module")
def runs(hip_lib_built, refs, tmp_path_factory):
    """{plan: arrays of child_plan} and {"buffers": arrays of child_buffers}, the five children running side by side, each under its
    own time limit."""
    return dm.start_children("test_second_depth_gpu", refs["path"], tmp_path_factory.mktemp("second_runs"))


@pytest.mark.parametrize("name", s2.SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_forward_returns_the_second_return(plan, name, runs, refs):
    """At every gap of the scene: on every decided pixel the range of the restatement's Gaussian comes back (a wrong neighbour differs
    by the gap or by metres, which no tolerance hides: every decided pixel is held to RTOL, none is excused), 0 where the rule finds no
    candidate; colour, occupancy and radii are the same child's default forward, bit for bit."""
    r = runs[plan]
    for gap in s2.gaps(name):
        ref, key = refs[name]["restated"][gap], _key(name, gap)
        dm.check_decided_pixels_return_the_restatements_range(f"{plan}.{key}", r[f"{key}.depth"][0], ref, ref["second_depth"], ref["has_second"])
        for k in ("color", "occ", "radii"):
            assert same_bits(r[f"{key}.{k}"], r[f"{name}.default0.{k}"]), (gap, k)
        if (name, gap) in BACKWARD:                                       # the scene's second forward under the mode is its first, bit for bit
            for k in IMAGE_KEYS:
                assert same_bits(r[f"{key}.{k}"], r[f"{key}0.{k}"]), (gap, k)


@pytest.mark.parametrize("W", [64, 250, 256])
@pytest.mark.parametrize("plan", list(PLANS))
def test_hand_placed_rays(plan, W, runs):
    """The rays whose answer is known by arithmetic (second_ref.placed; second_ref.ANSWERS writes them out for the gap unset and
    0.505 m).  Without the mode `second` is an unknown value and these pixels return the expected range: a point between the surfaces,
    never 0 where something was hit -- these assertions fail without the feature."""
    r = runs[plan]
    for gap in s2.PLACED_GAPS:
        got = r[f"{_key(f'second{W}', gap)}.depth"][0]
        want = s2.placed(W, gap)[1]
        for case, (x, y, rng, _) in want.items():
            assert got[y, x] == pytest.approx(rng, rel=1e-5), (case, gap, got[y, x], rng)
            if rng == 0.0:
                assert got[y, x] == 0.0, (case, gap)
            if gap in s2.GAPS:
                assert got[y, x] == pytest.approx(ANSWERS[case][s2.GAPS.index(gap)], rel=1e-5), (case, gap)
    x, y = s2.placed(W)[1]["single"][:2]
    assert r[f"second{W}.default0.depth"][0][y, x] > 1.0                  # (the default mode: range x weight, where `second` returns 0)


@pytest.mark.parametrize("case", BACKWARD, ids=BACKWARD_IDS)
@pytest.mark.parametrize("plan", list(PLANS))
def test_backward_matches_the_float64_autograd_of_the_restatement(plan, case, runs, refs):
    """All six gradient arrays against torch.autograd of the float64 forward whose depth is depth[second_id], upstream depth gradients
    masked on undecided pixels: util.parity, default tolerances, on median_ref.BACKWARD_SCENES at 0.505 m and one of them with the gap
    unset (their float32 budget is asserted by tests/test_median_depth_cpu.py in the default mode)."""
    name, gap = case
    dm.check_backward_against_float64(f"{plan}.{_key(name, gap)}", runs[plan], _key(name, gap), refs[name]["ref"][gap])


@pytest.mark.parametrize("case", BACKWARD, ids=BACKWARD_IDS)
@pytest.mark.parametrize("plan", list(PLANS))
def test_without_a_depth_gradient_the_backward_is_the_default_modes(plan, case, runs, refs):
    """dL/ddepth = 0: the blend's depth terms and the add to the picked Gaussian both vanish, and the gradients are the default mode's
    on the same scene within the backward's own run-to-run band (float atomics in scheduling order)."""
    name, gap = case
    dm.check_no_depth_gradient_gives_the_default_backward(f"{plan}.{_key(name, gap)}", runs[plan], _key(name, gap) + "0", f"{name}.default0",
                                                          refs[name]["oracle0_64"])


def test_depth_gradient_lands_on_exactly_one_gaussian(runs, refs):
    """second - second0 is the depth part alone: dL/dmeans3D rows differ exactly for the Gaussians that are some decided pixel's second
    return with a non-zero upstream gradient (one Gaussian per pixel), and colours / opacities carry none of it."""
    for plan in PLANS:
        for name, gap in BACKWARD:
            if name in mr.RANDOM:
                key = _key(name, gap)
                dm.check_depth_gradient_lands_on_one_gaussian(f"{plan}.{key}", runs[plan], key, key + "0", refs[name]["ref"][gap], "second_id",
                                                              refs[name]["oracle0_64"])


def test_buffer_sizes_and_values_of_the_switch(runs):
    """The buffers are a median forward's: only the image buffer grows, by the id plane (4 B per pixel, plus alignment), at either gap;
    `Second`, a trailing blank and `2` ask for the default sizes, as does a default forward after the mode has been used."""
    b = runs["buffers"]
    like_default = dict({value: b[f"sizes[{value}]"] for value in REJECTED}, default_after=b["default_after.sizes"])
    for gap in s2.GAPS:
        dm.check_buffer_sizes(b["never_set.sizes"], b[f"second[{s2.gap_tag(gap)}].sizes"], (b["sizes_median"], b["strongest_before.sizes"]), like_default,
                              H * mr.RANDOM[BUFFER_SCENE][2])


def test_the_id_plane_names_the_restatements_gaussian(runs, refs):
    """... on every decided pixel, 0xFFFFFFFF where there is no second return; and wherever the second return exists it is another
    Gaussian than the one the same child's `strongest` forward names."""
    b = runs["buffers"]
    strongest = b["strongest_before.id"].astype(np.int64)
    for gap in s2.GAPS:
        ref = refs[BUFFER_SCENE]["restated"][gap]
        tag = f"second[{s2.gap_tag(gap)}]"
        ids = dm.check_id_plane(f"G={s2.gap_tag(gap)}", b[f"{tag}.id"], ref, "second_id")
        exists = ids >= 0
        assert (ids[exists] != strongest.reshape(ids.shape)[exists]).all() and exists.sum() > 1000
        assert (b[f"{tag}.depth"][0][~exists] == 0).all() and (b[f"{tag}.depth"][0][exists] > 0).all()
        assert not same_bits(b[f"{tag}.depth"], b["never_set.depth"]) and not same_bits(b[f"{tag}.depth"], b["strongest_before.depth"])
    assert not same_bits(b["second[unset].id"], b["second[0.505].id"])          # (the gap does something)
    sid = refs[BUFFER_SCENE]["strongest"]
    assert (strongest.reshape(sid["decided"].shape)[sid["decided"]] == (sid["strongest_id"][sid["decided"]] & 0xFFFFFFFF)).all()


def test_second_forwards_leave_the_other_modes_alone(runs):
    """A `strongest` forward behind the `second` forwards is the one taken before them, bit for bit, id plane included; colour,
    occupancy and radii of every forward of the child are the first default forward's."""
    b = runs["buffers"]
    for k in IMAGE_KEYS + ("id", "sizes"):
        assert same_bits(b[f"strongest_after.{k}"], b[f"strongest_before.{k}"]), k
    for tag in ("strongest_before", "second[unset]", "second[0.505]", "default_after", "gap_alone", "strongest_with_gap"):
        for k in ("color", "occ", "radii"):
            assert same_bits(b[f"{tag}.{k}"], b[f"never_set.{k}"]), (tag, k)
    assert same_bits(b["default_after.depth"], b["never_set.depth"])


def test_the_gap_without_the_mode_changes_nothing(runs):
    """LIDARGS_RETURN_GAP without LIDARGS_DEPTH=second: buffer sizes and all outputs are bit-equal, under the default mode and under
    `strongest` (its id plane too)."""
    b = runs["buffers"]
    for k in IMAGE_KEYS + ("sizes",):
        assert same_bits(b[f"gap_alone.{k}"], b[f"never_set.{k}"]), k
    for k in IMAGE_KEYS + ("sizes", "id"):
        assert same_bits(b[f"strongest_with_gap.{k}"], b[f"strongest_before.{k}"]), k


def test_backward_twice_and_on_cloned_buffers_with_the_variables_unset(runs, refs):
    """The mode travels in the buffers and the gap is the forward's alone: forward under both variables, both removed, then backward,
    backward again and backward on clones of every saved tensor -- all the reference's gradients, and each other's within the
    run-to-run band."""
    dm.check_backward_twice_and_on_clones(runs["buffers"], refs[BUFFER_SCENE]["ref"][BUFFER_GAP])


def test_a_default_buffer_gets_the_default_gradients_after_a_second_forward(runs, refs):
    """The buffer's mode bit decides, not the process (depth_modes.check_default_buffer_after_a_picked_forward)."""
    up = np.load(refs["path"])
    grads = (up[f"{BUFFER_SCENE}.gc"], up[f"{_key(BUFFER_SCENE, BUFFER_GAP)}.gd_masked"], up[f"{BUFFER_SCENE}.go"])
    dm.check_default_buffer_after_a_picked_forward(runs["buffers"], refs[BUFFER_SCENE]["scene"], refs[BUFFER_SCENE]["W"], grads)


@pytest.mark.parametrize("case", list(REFUSING))
def test_entry_points_the_mode_does_not_cover_refuse_it(case, runs):
    """The surfel variant, shells and wedges, the enqueue-only forward, and lidargs_forward under LIDARGS_DETERMINISTIC=1 as well: a
    RuntimeError naming the variable and the entry point.  Without the switch they run, before and after."""
    dm.check_refusal(case, runs["buffers"])
