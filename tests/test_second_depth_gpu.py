"""LIDARGS_DEPTH=second on the GPU: the second-return range of the 3-D rasterizer, forward and backward (the rule: csrc/switches.h
second_depth_requested), with LIDARGS_RETURN_GAP unset and set.

Reference: tests/second_ref.py -- the rule restated on tests/strongest_ref.py's table of the CPU oracle's forward state, and the
float64 autograd of a forward whose depth is depth[second_id].  A pixel whose strongest return is undecided, whose two heaviest
candidates are within 1e-3 of each other or which has an entry within 1 mm of the gap's edge is undecided (second_ref.py says when):
it gives no vote in the forward and gets a zero upstream depth gradient; tests/test_second_depth_cpu.py holds every scene and gap
used here to at most 2 % of them.

Scenes (second_ref.SCENES): those of the strongest tests and the hand-placed rays of second_ref.placed, 16 rows x 64 / 250 / 256
columns, at the gap unset and 0.505 m (the hand-placed rays of this mode at 2.005 m as well).  Built like
tests/test_strongest_depth_gpu.py, with tests/test_median_depth_gpu.py's plans, frame helper and refusing forwards as they are: every
scene runs in four child processes -- LIDARGS_FUSED = 0 / 1 x LIDARGS_TILE_ROWS = 4 / 32 -- started together; a fifth child does what
hangs on the buffers and the refusals.  Both variables are read at every forward and are set inside the children only.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import median_ref as mr
import second_ref as s2
import strongest_ref as sr
import test_median_depth_gpu as tm
from test_median_depth_gpu import PLANS, REFUSING, SWITCH, same_bits
from test_second_depth_cpu import ANSWERS
from util import (FLOOR, GRAD_KEYS_SR, RTOL, hip_forward_backward, oracle_backward_exact_sums, oracle_forward_backward, parity, parity_or_closer,
                  run_child)

pytestmark = pytest.mark.gpu

H = s2.H
GAP = "LIDARGS_RETURN_GAP"
IMAGE_KEYS = ("color", "depth", "occ", "radii")
BUFFER_SCENE = "shell256"
BUFFER_GAP = 0.505
CHILD_SECONDS = 300
BACKWARD = [(name, 0.505) for name in s2.BACKWARD_SCENES] + [(s2.BACKWARD_UNSET, None)]      # (scene, gap) of the backward tests
BACKWARD_IDS = [f"{name}-G={s2.gap_tag(gap)}" for name, gap in BACKWARD]
ENTRY = {"surfel": "lidargs_surfel_forward", "shell_world_of_one": "lidargs_forward_shell", "wedge_world_of_one": "lidargs_forward_wedge",
         "enqueue_only": "lidargs_forward_enqueue", "deterministic_and_median": "lidargs_forward"}


def _with(depth, gap, fn):
    """fn() under LIDARGS_DEPTH = depth and LIDARGS_RETURN_GAP = gap (None: unset); both unset behind it."""
    if gap is None:
        os.environ.pop(GAP, None)
    else:
        os.environ[GAP] = gap if isinstance(gap, str) else f"{gap:g}"
    try:
        return tm._with_switch(depth, fn)
    finally:
        os.environ.pop(GAP, None)


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
        r = _with(None, None, lambda: hip_forward_backward(scene, W, H, nodepth if backward else None))
        res.update({f"{name}.default0.{k}": r[k] for k in IMAGE_KEYS + (GRAD_KEYS_SR if backward else ())})
        for gap in s2.gaps(name):
            key = _key(name, gap)
            if (name, gap) in BACKWARD:
                masked = (nodepth[0], up[f"{key}.gd_masked"], nodepth[2])
                r = _with("second", gap, lambda: hip_forward_backward(scene, W, H, masked))
                res.update({f"{key}.{k}": r[k] for k in IMAGE_KEYS + GRAD_KEYS_SR})
                r = _with("second", gap, lambda: hip_forward_backward(scene, W, H, nodepth))
                res.update({f"{key}0.{k}": r[k] for k in IMAGE_KEYS + GRAD_KEYS_SR})
            else:
                r = _with("second", gap, lambda: hip_forward_backward(scene, W, H))
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
    fr = tm._Frame(name, (up[f"{name}.gc"], up[f"{_key(name, BUFFER_GAP)}.gd_masked"], up[f"{name}.go"]))
    res = {}
    sizes = lambda fwd: np.array([int(t.numel()) for t in fwd[5:8]], np.int64)
    images = lambda fwd: {k: fwd[i].cpu().numpy() for k, i in (("color", 1), ("depth", 2), ("occ", 3), ("radii", 4))}

    def plane(fwd, n_img):
        off = (n_img - 128 + 127) // 128 * 128                    # (lidargs_common.h img_carve: the plane starts at the next 128-byte boundary)
        p = fwd[7][off:off + 4 * H * fr.W].cpu().numpy()          # (shorter than H x W words where the forward asked for no plane: the test says so)
        return p[:p.size // 4 * 4].view(np.uint32)

    def record(tag, fwd, n_img, with_plane=True):
        res[f"{tag}.sizes"] = sizes(fwd)
        res.update({f"{tag}.{k}": v for k, v in images(fwd).items()})
        if with_plane:
            res[f"{tag}.id"] = plane(fwd, n_img)

    plain = fr.forward()
    n_img = int(sizes(plain)[2])
    record("never_set", plain, n_img, False)
    res.update({f"before.{k}": v for k, v in fr.backward(plain).items()})     # (no such forward yet in this process: the default launches)
    for value in ("Second", "second ", "2"):
        res[f"sizes[{value}]"] = _with(value, None, lambda: sizes(fr.forward()))
    record("gap_alone", _with(None, "0.505", fr.forward), n_img, False)         # LIDARGS_RETURN_GAP without the mode: nothing changes
    record("strongest_before", _with("strongest", None, fr.forward), n_img)
    record("strongest_with_gap", _with("strongest", "0.505", fr.forward), n_img)
    on = None
    for gap in s2.GAPS:
        fwd = _with("second", gap, fr.forward)
        record(f"second[{s2.gap_tag(gap)}]", fwd, n_img)
        if gap == BUFFER_GAP:
            on = fwd
    record("strongest_after", _with("strongest", None, fr.forward), n_img)
    res["sizes_median"] = _with("median", None, lambda: sizes(fr.forward()))
    # both variables are unset from here on: the mode travels in the buffers, the gap nowhere
    for what, fn in (("first", lambda: fr.backward(on)), ("second", lambda: fr.backward(on)), ("cloned", lambda: fr.backward(on, clone=True))):
        res.update({f"{what}.{k}": v for k, v in fn().items()})
    off_again = fr.forward()                                      # a default forward in a process that has made such buffers
    record("default_after", off_again, n_img, False)
    res.update({f"default_after.{k}": v for k, v in fr.backward(off_again).items()})
    res.update({f"third.{k}": v for k, v in fr.backward(on).items()})     # ... and the second-return buffers again behind it
    for case, forward in REFUSING.items():
        ok_before = bool(np.isfinite(_with(None, None, forward)).all()) if case != "deterministic_and_median" else True
        try:
            _with("second", "0.505", forward)
            msg = "no error"
        except RuntimeError as e:
            msg = "RuntimeError: " + str(e)
        ok_after = bool(np.isfinite(_with(None, None, forward)).all())
        res[f"refusal.{case}"] = np.array([msg, str(ok_before), str(ok_after)])
    np.savez(out, **res)
    print("OK")


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """Per scene: the restatement at every gap of the scene; per (scene, gap) of BACKWARD the float64 reference gradients for upstream
    gradients whose depth part is masked on undecided pixels (second_ref.reference), and per backward scene the CPU oracle's
    default-mode backward for the same upstream gradients without a depth part, with its exact sums.  Computed once; the upstream
    gradients go to the children in a file."""
    from oracle import lgo
    out, up = {}, {}
    for name in s2.SCENES:
        scene, W = s2.scene(name)
        gc, gd, go = s2.upstream(name)
        f = lgo.forward(scene["means3D"], scene["colors"], scene["opacities"], scene["scales"], scene["rotations"], scene["viewmatrix"],
                        scene["beams"], W, H, bg=scene["bg"])
        rs = sr.restate(f, scene, W, H)
        entry = dict(scene=scene, W=W, strongest=rs, restated={gap: s2.restate(f, rs, gap) for gap in s2.gaps(name)}, ref={})
        up.update({f"{name}.gc": gc, f"{name}.go": go})
        if name in s2.BACKWARD_SCENES:
            nodepth = (gc, np.zeros_like(gd), go)
            entry["oracle0"] = oracle_forward_backward(scene, W, H, nodepth)
            entry["oracle0_64"] = oracle_backward_exact_sums(entry["oracle0"], nodepth)
        for gap in s2.gaps(name):
            if (name, gap) in BACKWARD:
                entry["ref"][gap] = s2.reference(scene, W, H, (gc, gd, go), gap, f=f)
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
    d = tmp_path_factory.mktemp("second_runs")
    code = "import os\nos.environ.pop(%r, None)\nos.environ.pop(%r, None)\nimport test_second_depth_gpu as t\nt.%s(sys.argv[1], sys.argv[2])"
    jobs = {plan: (code % (SWITCH, GAP, "child_plan"), env) for plan, env in PLANS.items()}
    jobs["buffers"] = (code % (SWITCH, GAP, "child_buffers"), {})
    outs = {k: str(d / f"{k}.npz") for k in jobs}
    with ThreadPoolExecutor(len(jobs)) as pool:
        fut = [pool.submit(run_child, body, env, (refs["path"], outs[k]), CHILD_SECONDS) for k, (body, env) in jobs.items()]
        for f in fut:
            f.result()
    return {k: dict(np.load(o)) for k, o in outs.items()}


@pytest.mark.parametrize("name", s2.SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_forward_returns_the_second_return(plan, name, runs, refs):
    """At every gap of the scene: on every decided pixel the range of the restatement's Gaussian comes back (a wrong neighbour differs
    by the gap or by metres, which no tolerance hides: every decided pixel is held to RTOL, none is excused), 0 where the rule finds no
    candidate; colour, occupancy and radii are the same child's default forward, bit for bit."""
    r = runs[plan]
    for gap in s2.gaps(name):
        ref, key = refs[name]["restated"][gap], _key(name, gap)
        got, dec, want = r[f"{key}.depth"][0], ref["decided"], ref["second_depth"]
        assert dec.sum() >= 0.98 * ref["has_taker"].sum()
        err = np.abs(got[dec] - want[dec]) / (np.abs(want[dec]) + FLOOR * np.abs(want[dec]).max())
        print(f"G={s2.gap_tag(gap)}: decided pixels {int(dec.sum())} of {dec.size}, worst error {err.max():.2e}, wrong Gaussians: {int((err > 1e-3).sum())}")
        assert err.max() <= RTOL, f"G={s2.gap_tag(gap)}: {int((err > RTOL).sum())} decided pixels return another range than the restatement's Gaussian's"
        assert (got[~ref["has_second"] & dec] == 0).all()
        for k in ("color", "occ", "radii"):
            assert same_bits(r[f"{key}.{k}"], r[f"{name}.default0.{k}"]), (gap, k)
        if (name, gap) in BACKWARD:                                       # the scene's second forward under the mode is its first, bit for bit
            for k in IMAGE_KEYS:
                assert same_bits(r[f"{key}.{k}"], r[f"{key}0.{k}"]), (gap, k)


@pytest.mark.parametrize("W", [64, 250, 256])
@pytest.mark.parametrize("plan", list(PLANS))
def test_hand_placed_rays(plan, W, runs):
    """The rays whose answer is known by arithmetic (second_ref.placed; tests/test_second_depth_cpu.py ANSWERS writes them out for the
    gap unset and 0.505 m).  Without the mode `second` is an unknown value and these pixels return the expected range: a point between
    the surfaces, never 0 where something was hit -- these assertions fail without the feature."""
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
    r, ref, key = runs[plan], refs[name]["ref"][gap], _key(name, gap)
    over = lambda got, want: int((np.abs(got - want) / (np.abs(want) + FLOOR * np.abs(want).max() + 1e-30) > RTOL).sum())
    failed = []
    for k in GRAD_KEYS_SR:
        try:
            parity(f"{plan}.{key}.{k}", r[f"{key}.{k}"], ref[k])
        except AssertionError as e:
            failed.append(f"{e} [entries over {RTOL:g}: {over(r[f'{key}.{k}'], ref[k])}]")
    assert not failed, failed


@pytest.mark.parametrize("case", BACKWARD, ids=BACKWARD_IDS)
@pytest.mark.parametrize("plan", list(PLANS))
def test_without_a_depth_gradient_the_backward_is_the_default_modes(plan, case, runs, refs):
    """dL/ddepth = 0: the blend's depth terms and the add to the picked Gaussian both vanish, and the gradients are the default mode's
    on the same scene within the backward's own run-to-run band (float atomics in scheduling order)."""
    name, gap = case
    r = runs[plan]
    for k in GRAD_KEYS_SR:
        parity_or_closer(f"{plan}.{_key(name, gap)}.{k} (no depth gradient)", r[f"{_key(name, gap)}0.{k}"], r[f"{name}.default0.{k}"],
                         refs[name]["oracle0_64"][k])


def test_depth_gradient_lands_on_exactly_one_gaussian(runs, refs):
    """second - second0 is the depth part alone: dL/dmeans3D rows differ exactly for the Gaussians that are some decided pixel's second
    return with a non-zero upstream gradient (one Gaussian per pixel), and colours / opacities carry none of it."""
    for plan in PLANS:
        for name, gap in BACKWARD:
            if name not in mr.RANDOM:
                continue
            r, ref, key = runs[plan], refs[name]["ref"][gap], _key(name, gap)
            gd = ref["dL_ddepth_masked"][0]
            ok = (ref["second_id"] >= 0) & (gd != 0)
            want = np.zeros(ref["dL_dmeans3D"].shape[0])
            np.add.at(want, ref["second_id"][ok], gd[ok].astype(np.float64))
            part = r[f"{key}.dL_dmeans3D"].astype(np.float64) - r[f"{key}0.dL_dmeans3D"]
            moved = np.abs(part).max(1)
            scale = np.abs(r[f"{key}0.dL_dmeans3D"]).max(1) + np.abs(want)
            assert not (moved[want == 0] > 1e-3 * (scale[want == 0] + 1e-6)).any(), (plan, key)
            big = np.abs(want) > 1e-2 * np.abs(want).max()
            assert (moved[big] > 0).all() and big.sum() >= 20, (plan, key)
            np.testing.assert_allclose(np.linalg.norm(part, axis=1)[big], np.abs(want[big]), rtol=2e-2)   # |d range / d mean| = 1 (differences of float32 sums)
            for k in ("dL_dcolors", "dL_dopacity"):
                parity_or_closer(f"{plan}.{key}.{k} (depth part)", r[f"{key}.{k}"], r[f"{key}0.{k}"], refs[name]["oracle0_64"][k])


def test_buffer_sizes_and_values_of_the_switch(runs):
    """The buffers are a median forward's: only the image buffer grows, by the id plane (4 B per pixel, plus alignment), at either gap;
    `Second`, a trailing blank and `2` ask for the default sizes, as does a default forward after the mode has been used."""
    b = runs["buffers"]
    N = H * mr.RANDOM[BUFFER_SCENE][2]
    for gap in s2.GAPS:
        on = b[f"second[{s2.gap_tag(gap)}].sizes"]
        extra = on - b["never_set.sizes"]
        assert extra[0] == 0 and extra[1] == 0 and 4 * N <= extra[2] <= 4 * N + 256, extra
        assert (on == b["sizes_median"]).all() and (on == b["strongest_before.sizes"]).all()
    for value in ("Second", "second ", "2"):
        assert (b[f"sizes[{value}]"] == b["never_set.sizes"]).all(), value
    assert (b["default_after.sizes"] == b["never_set.sizes"]).all()


def test_the_id_plane_names_the_restatements_gaussian(runs, refs):
    """... on every decided pixel, 0xFFFFFFFF where there is no second return; and wherever the second return exists it is another
    Gaussian than the one the same child's `strongest` forward names."""
    b = runs["buffers"]
    strongest = b["strongest_before.id"].astype(np.int64)
    for gap in s2.GAPS:
        ref = refs[BUFFER_SCENE]["restated"][gap]
        dec = ref["decided"]
        tag = f"second[{s2.gap_tag(gap)}]"
        assert b[f"{tag}.id"].size == dec.size, "the image buffer has no id plane"
        ids = b[f"{tag}.id"].astype(np.int64).reshape(dec.shape)
        exists = ids != 0xFFFFFFFF
        assert (ids[exists] != strongest.reshape(dec.shape)[exists]).all() and exists.sum() > 1000
        ids[~exists] = -1
        assert dec.sum() >= 0.98 * ref["has_taker"].sum()
        wrong = int((ids[dec] != ref["second_id"][dec]).sum())
        print(f"G={s2.gap_tag(gap)}: decided pixels {int(dec.sum())}, other Gaussian than the restatement's: {wrong}")
        assert wrong == 0
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
    b, ref = runs["buffers"], refs[BUFFER_SCENE]["ref"][BUFFER_GAP]
    for k in GRAD_KEYS_SR:
        for what in ("first", "second", "cloned", "third"):
            parity(f"buffers.{what}.{k}", b[f"{what}.{k}"], ref[k], verbose=False)
        for what in ("second", "cloned", "third"):
            parity(f"buffers.{what} against first.{k}", b[f"{what}.{k}"], b[f"first.{k}"], verbose=False)
    assert np.abs(b["first.dL_dmeans3D"] - b["before.dL_dmeans3D"]).max() > 1e-2 * np.abs(b["first.dL_dmeans3D"]).max()   # (the modes do differ)


def test_a_default_buffer_gets_the_default_gradients_after_a_second_forward(runs, refs):
    """The buffer's mode bit decides, not the process: a default forward's backward after the process has made second-return buffers
    is the default backward of before -- the CPU oracle's gradients for the same upstream gradients, depth part included."""
    b = runs["buffers"]
    scene, W = refs[BUFFER_SCENE]["scene"], refs[BUFFER_SCENE]["W"]
    up = np.load(refs["path"])
    grads = (up[f"{BUFFER_SCENE}.gc"], up[f"{_key(BUFFER_SCENE, BUFFER_GAP)}.gd_masked"], up[f"{BUFFER_SCENE}.go"])
    ora = oracle_forward_backward(scene, W, H, grads)
    ora64 = oracle_backward_exact_sums(ora, grads)
    for k in GRAD_KEYS_SR:
        for what in ("before", "default_after"):
            parity_or_closer(f"buffers.{what}.{k}", b[f"{what}.{k}"], ora[k], ora64[k])
        parity_or_closer(f"buffers.default_after against before.{k}", b[f"default_after.{k}"], b[f"before.{k}"], ora64[k])


@pytest.mark.parametrize("case", list(REFUSING))
def test_entry_points_the_mode_does_not_cover_refuse_it(case, runs):
    """The surfel variant, shells and wedges, the enqueue-only forward, and lidargs_forward under LIDARGS_DETERMINISTIC=1 as well: a
    RuntimeError naming the variable and the entry point.  Without the switch they run, before and after."""
    msg, ok_before, ok_after = runs["buffers"][f"refusal.{case}"]
    assert msg.startswith("RuntimeError") and SWITCH in msg and ENTRY[case] in msg, msg
    assert ok_before == "True" and ok_after == "True"
