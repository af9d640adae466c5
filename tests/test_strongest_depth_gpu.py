"""LIDARGS_DEPTH=strongest on the GPU: the strongest-return range of the 3-D rasterizer, forward and backward (DESIGN.md "Median-range
depth", the strongest-return rule).

Reference: tests/strongest_ref.py -- the rule restated on the CPU oracle's forward state, and the float64 autograd of a forward whose
depth is depth[strongest_id].  A pixel whose decision sits within rounding of a threshold or whose two largest weights are within 1e-3
of each other is undecided (strongest_ref.py says when): it gives no vote in the forward and gets a zero upstream depth gradient;
tests/test_strongest_depth_cpu.py holds every scene used here to at most 2 % of them.

Scenes (strongest_ref.SCENES): those of the median tests and the hand-placed rays of strongest_ref.placed, 16 rows x 64 / 250 / 256
columns.  Built like tests/test_median_depth_gpu.py, whose plans, frame helper and refusing forwards are used as they are: every scene
runs in four child processes -- LIDARGS_FUSED = 0 / 1 x LIDARGS_TILE_ROWS = 4 / 32 -- started together; a fifth child does what hangs
on the buffers and the refusals.  LIDARGS_DEPTH is read at every forward and is set inside the children only.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import median_ref as mr
import strongest_ref as sr
import test_median_depth_gpu as tm
from test_median_depth_gpu import PLANS, REFUSING, SWITCH, same_bits
from util import (FLOOR, GRAD_KEYS_SR, RTOL, hip_forward_backward, oracle_backward_exact_sums, oracle_forward_backward, parity, parity_or_closer,
                  run_child)

pytestmark = pytest.mark.gpu

H = sr.H
IMAGE_KEYS = ("color", "depth", "occ", "radii")
BUFFER_SCENE = "shell256"
CHILD_SECONDS = 300


def child_plan(refs, out):
    """One child process: every scene's forward + backward under `strongest` and in the default mode, with the reference's masked depth
    gradient and with none (the second being the second strongest forward of the scene); the hand-placed rays under `median` as well."""
    assert SWITCH not in os.environ
    up = np.load(refs)
    res = {}
    for name in sr.SCENES:
        scene, W = sr.scene(name)
        masked = (up[f"{name}.gc"], up[f"{name}.gd_masked"], up[f"{name}.go"])
        nodepth = (masked[0], np.zeros_like(masked[1]), masked[2])
        for mode, value in (("strongest", "strongest"), ("default", None)):
            r = tm._with_switch(value, lambda: hip_forward_backward(scene, W, H, masked))
            res.update({f"{name}.{mode}.{k}": r[k] for k in IMAGE_KEYS + GRAD_KEYS_SR})
            r = tm._with_switch(value, lambda: hip_forward_backward(scene, W, H, nodepth))
            res.update({f"{name}.{mode}0.{k}": r[k] for k in IMAGE_KEYS + GRAD_KEYS_SR})
        if name in sr.PLACED:
            res[f"{name}.median.depth"] = tm._with_switch("median", lambda: hip_forward_backward(scene, W, H))["depth"]
    np.savez(out, **res)
    print("OK")


def child_buffers(refs, out):
    """The fifth child: buffer sizes, the id plane, backward twice / on clones with the variable unset, a default forward's backward in
    a process that has made such buffers, the values of the switch, and the refusals."""
    assert SWITCH not in os.environ
    up = np.load(refs)
    name = BUFFER_SCENE
    fr = tm._Frame(name, (up[f"{name}.gc"], up[f"{name}.gd_masked"], up[f"{name}.go"]))
    res = {}
    sizes = lambda fwd: np.array([int(t.numel()) for t in fwd[5:8]], np.int64)
    plain = fr.forward()
    res["sizes_never_set"] = sizes(plain)
    res["never_set.depth"] = plain[2].cpu().numpy()
    before = fr.backward(plain)                                   # (no such forward yet in this process: the default launches)
    res.update({f"before.{k}": v for k, v in before.items()})
    for value in ("", "Strongest", "strongest ", "1", "expected"):
        res[f"sizes[{value}]"] = tm._with_switch(value, lambda: sizes(fr.forward()))
    on = tm._with_switch("strongest", fr.forward)
    res["sizes_switch_on"] = sizes(on)
    res["strongest.depth"] = on[2].cpu().numpy()
    n_img = int(res["sizes_never_set"][2])
    off = (n_img - 128 + 127) // 128 * 128                        # (lidargs_common.h img_carve: the plane starts at the next 128-byte boundary)
    plane = on[7][off:off + 4 * H * fr.W].cpu().numpy()           # (shorter than H x W words where the forward asked for no plane: the test says so)
    res["strongest_id"] = plane[:plane.size // 4 * 4].view(np.uint32)
    # the variable is unset from here on: the mode travels in the buffers
    for what, fn in (("first", lambda: fr.backward(on)), ("second", lambda: fr.backward(on)), ("cloned", lambda: fr.backward(on, clone=True))):
        res.update({f"{what}.{k}": v for k, v in fn().items()})
    off_again = fr.forward()                                      # a default forward in a process that has made such buffers
    res["sizes_set_and_unset"] = sizes(off_again)
    res.update({f"default_after.{k}": v for k, v in fr.backward(off_again).items()})
    res.update({f"default_after_cloned.{k}": v for k, v in fr.backward(off_again, clone=True).items()})
    res.update({f"third.{k}": v for k, v in fr.backward(on).items()})     # ... and the strongest buffers again behind it
    res["sizes_median"] = tm._with_switch("median", lambda: sizes(fr.forward()))
    for case, forward in REFUSING.items():
        ok_before = bool(np.isfinite(tm._with_switch(None, forward)).all()) if case != "deterministic_and_median" else True
        try:
            tm._with_switch("strongest", forward)
            msg = "no error"
        except RuntimeError as e:
            msg = "RuntimeError: " + str(e)
        ok_after = bool(np.isfinite(tm._with_switch(None, forward)).all())
        res[f"refusal.{case}"] = np.array([msg, str(ok_before), str(ok_after)])
    np.savez(out, **res)
    print("OK")


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """Per scene: the restatement and the float64 reference gradients for upstream gradients whose depth part is masked on undecided
    pixels (strongest_ref.reference), and the CPU oracle's default-mode backward for the same upstream gradients without a depth part,
    with its exact sums.  Computed once; the upstream gradients go to the children in a file."""
    out, up = {}, {}
    for name in sr.SCENES:
        scene, W = sr.scene(name)
        gc, gd, go = sr.upstream(name)
        ref = sr.reference(scene, W, H, (gc, gd, go))
        nodepth = (gc, np.zeros_like(gd), go)
        ora = oracle_forward_backward(scene, W, H, nodepth)
        ora64 = oracle_backward_exact_sums(ora, nodepth)
        ref0 = sr.reference(scene, W, H, nodepth, f=ref["fwd"]) if name in sr.BACKWARD_SCENES else None
        out[name] = dict(scene=scene, W=W, ref=ref, ref0=ref0, oracle0=ora, oracle0_64=ora64)
        up.update({f"{name}.gc": gc, f"{name}.gd_masked": ref["dL_ddepth_masked"], f"{name}.go": go})
    path = str(tmp_path_factory.mktemp("strongest") / "upstream.npz")
    np.savez(path, **up)
    out["path"] = path
    return out


@pytest.fixture(scope="module")
def runs(hip_lib_built, refs, tmp_path_factory):
    """{plan: arrays of child_plan} and {"buffers": arrays of child_buffers}, the five children running side by side, each under its
    own time limit."""
    d = tmp_path_factory.mktemp("strongest_runs")
    code = "import os\nos.environ.pop(%r, None)\nimport test_strongest_depth_gpu as t\nt.%s(sys.argv[1], sys.argv[2])"
    jobs = {plan: (code % (SWITCH, "child_plan"), env) for plan, env in PLANS.items()}
    jobs["buffers"] = (code % (SWITCH, "child_buffers"), {})
    outs = {k: str(d / f"{k}.npz") for k in jobs}
    with ThreadPoolExecutor(len(jobs)) as pool:
        fut = [pool.submit(run_child, body, env, (refs["path"], outs[k]), CHILD_SECONDS) for k, (body, env) in jobs.items()]
        for f in fut:
            f.result()
    return {k: dict(np.load(o)) for k, o in outs.items()}


@pytest.mark.parametrize("name", sr.SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_forward_returns_the_strongest_return(plan, name, runs, refs):
    """On every decided pixel the range of the restatement's Gaussian comes back (a wrong neighbour differs by metres, which no
    tolerance hides: every decided pixel is held to RTOL, none is excused), 0 where no pixel takes anything; colour, occupancy and
    radii are the same child's default forward, bit for bit; the scene's second strongest forward is the first, bit for bit."""
    r, ref = runs[plan], refs[name]["ref"]
    got, dec = r[f"{name}.strongest.depth"][0], ref["decided"]
    want = ref["strongest_depth"]
    assert dec.sum() >= 0.98 * ref["has_taker"].sum()
    err = np.abs(got[dec] - want[dec]) / (np.abs(want[dec]) + FLOOR * np.abs(want[dec]).max())
    print(f"decided pixels: {int(dec.sum())} of {dec.size}, worst error {err.max():.2e}, wrong Gaussians: {int((err > 1e-3).sum())}")
    assert err.max() <= RTOL, f"{int((err > RTOL).sum())} decided pixels return another range than the restatement's Gaussian's"
    assert (got[~ref["has_taker"] & dec] == 0).all()
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
    r, ref, ref0 = runs[plan], refs[name]["ref"], refs[name]["ref0"]
    over = lambda got, want: int((np.abs(got - want) / (np.abs(want) + FLOOR * np.abs(want).max() + 1e-30) > RTOL).sum())
    failed = []
    for k in GRAD_KEYS_SR:
        try:
            parity(f"{plan}.{name}.{k}", r[f"{name}.strongest.{k}"], ref[k])
        except AssertionError as e:
            failed.append(f"{e} [entries over {RTOL:g}: strongest mode {over(r[f'{name}.strongest.{k}'], ref[k])}, default mode without a depth "
                          f"gradient {over(r[f'{name}.default0.{k}'], ref0[k])}, CPU oracle {over(refs[name]['oracle0'][k], ref0[k])}]")
    assert not failed, failed


@pytest.mark.parametrize("name", sr.SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_without_a_depth_gradient_the_backward_is_the_default_modes(plan, name, runs, refs):
    """dL/ddepth = 0: the blend's depth terms and the add to the picked Gaussian both vanish, and the gradients are the default mode's
    on the same scene within the backward's own run-to-run band (float atomics in scheduling order)."""
    r = runs[plan]
    for k in GRAD_KEYS_SR:
        parity_or_closer(f"{plan}.{name}.{k} (no depth gradient)", r[f"{name}.strongest0.{k}"], r[f"{name}.default0.{k}"], refs[name]["oracle0_64"][k])


def test_depth_gradient_lands_on_exactly_one_gaussian(runs, refs):
    """strongest - strongest0 is the depth part alone: dL/dmeans3D rows differ exactly for the Gaussians that are some decided pixel's
    strongest return with a non-zero upstream gradient (one Gaussian per pixel), and colours / opacities carry none of it."""
    for plan in PLANS:
        for name in mr.RANDOM:
            r, ref = runs[plan], refs[name]["ref"]
            gd = ref["dL_ddepth_masked"][0]
            ok = (ref["strongest_id"] >= 0) & (gd != 0)
            want = np.zeros(ref["dL_dmeans3D"].shape[0])
            np.add.at(want, ref["strongest_id"][ok], gd[ok].astype(np.float64))
            part = r[f"{name}.strongest.dL_dmeans3D"].astype(np.float64) - r[f"{name}.strongest0.dL_dmeans3D"]
            moved = np.abs(part).max(1)
            scale = np.abs(r[f"{name}.strongest0.dL_dmeans3D"]).max(1) + np.abs(want)
            assert not (moved[want == 0] > 1e-3 * (scale[want == 0] + 1e-6)).any(), (plan, name)
            big = np.abs(want) > 1e-2 * np.abs(want).max()
            assert (moved[big] > 0).all() and big.sum() >= 20, (plan, name)
            np.testing.assert_allclose(np.linalg.norm(part, axis=1)[big], np.abs(want[big]), rtol=2e-2)   # |d range / d mean| = 1 (differences of float32 sums)
            for k in ("dL_dcolors", "dL_dopacity"):
                parity_or_closer(f"{plan}.{name}.{k} (depth part)", r[f"{name}.strongest.{k}"], r[f"{name}.strongest0.{k}"], refs[name]["oracle0_64"][k])


def test_buffer_sizes_and_values_of_the_switch(runs):
    """The buffers are a median forward's: only the image buffer grows, by the id plane (4 B per pixel, plus alignment); unset, empty
    and any value but the literal -- `Strongest` and a trailing blank among them -- ask for the default sizes, also after the mode has
    been used in the process."""
    b = runs["buffers"]
    extra = b["sizes_switch_on"] - b["sizes_never_set"]
    N = H * mr.RANDOM[BUFFER_SCENE][2]
    assert extra[0] == 0 and extra[1] == 0 and 4 * N <= extra[2] <= 4 * N + 256, extra
    assert (b["sizes_switch_on"] == b["sizes_median"]).all()
    for value in ("", "Strongest", "strongest ", "1", "expected"):
        assert (b[f"sizes[{value}]"] == b["sizes_never_set"]).all(), value
    assert (b["sizes_set_and_unset"] == b["sizes_never_set"]).all()


def test_the_id_plane_names_the_restatements_gaussian(runs, refs):
    b, ref = runs["buffers"], refs[BUFFER_SCENE]["ref"]
    dec = ref["decided"]
    assert b["strongest_id"].size == dec.size, "the image buffer has no id plane"
    ids = b["strongest_id"].astype(np.int64).reshape(dec.shape)
    ids[ids == 0xFFFFFFFF] = -1
    assert dec.sum() >= 0.98 * ref["has_taker"].sum() and (ref["strongest_id"] >= 0).sum() > 1000
    wrong = int((ids[dec] != ref["strongest_id"][dec]).sum())
    print(f"decided pixels {int(dec.sum())}, other Gaussian than the restatement's: {wrong}")
    assert wrong == 0
    assert not same_bits(b["strongest.depth"], b["never_set.depth"])


def test_backward_twice_and_on_cloned_buffers_with_the_variable_unset(runs, refs):
    """The mode travels in the buffers: forward under the switch, variable removed, then backward, backward again and backward on clones
    of every saved tensor -- all the reference's gradients, and each other's within the run-to-run band."""
    b, ref = runs["buffers"], refs[BUFFER_SCENE]["ref"]
    for k in GRAD_KEYS_SR:
        for what in ("first", "second", "cloned", "third"):
            parity(f"buffers.{what}.{k}", b[f"{what}.{k}"], ref[k], verbose=False)
        for what in ("second", "cloned", "third"):
            parity(f"buffers.{what} against first.{k}", b[f"{what}.{k}"], b[f"first.{k}"], verbose=False)
    assert np.abs(b["first.dL_dmeans3D"] - b["before.dL_dmeans3D"]).max() > 1e-2 * np.abs(b["first.dL_dmeans3D"]).max()   # (the modes do differ)


def test_a_default_buffer_gets_the_default_gradients_after_a_strongest_forward(runs, refs):
    """The buffer's mode bit decides, not the process: a default forward's backward after the process has made strongest buffers is the
    default backward of before -- the CPU oracle's gradients for the same upstream gradients, depth part included."""
    b = runs["buffers"]
    scene, W = refs[BUFFER_SCENE]["scene"], refs[BUFFER_SCENE]["W"]
    up = np.load(refs["path"])
    grads = (up[f"{BUFFER_SCENE}.gc"], up[f"{BUFFER_SCENE}.gd_masked"], up[f"{BUFFER_SCENE}.go"])
    ora = oracle_forward_backward(scene, W, H, grads)
    ora64 = oracle_backward_exact_sums(ora, grads)
    for k in GRAD_KEYS_SR:
        for what in ("before", "default_after", "default_after_cloned"):
            parity_or_closer(f"buffers.{what}.{k}", b[f"{what}.{k}"], ora[k], ora64[k])
        parity_or_closer(f"buffers.default_after against before.{k}", b[f"default_after.{k}"], b[f"before.{k}"], ora64[k])


@pytest.mark.parametrize("case", list(REFUSING))
def test_entry_points_the_mode_does_not_cover_refuse_it(case, runs):
    """The surfel variant, shells and wedges, the enqueue-only forward, and lidargs_forward under LIDARGS_DETERMINISTIC=1 as well: a
    RuntimeError naming the variable.  Without the switch they run, before and after."""
    msg, ok_before, ok_after = runs["buffers"][f"refusal.{case}"]
    assert msg.startswith("RuntimeError") and SWITCH in msg, msg
    assert ok_before == "True" and ok_after == "True"
