"""LIDARGS_DEPTH=median on the GPU: the median range of the 3-D rasterizer, forward and backward (DESIGN.md "Median-range depth").

Reference: tests/median_ref.py -- the rule restated on the CPU oracle's forward state, and the float64 autograd of a forward whose depth
is depth[median_id].  A pixel whose decision sits within rounding of a threshold is undecided (median_ref.py says when): it gives no vote
in the forward and gets a zero upstream depth gradient; tests/test_median_depth_cpu.py holds every scene used here to at most 2 % of them.

Scenes (median_ref.SCENES): four random ones and the hand-placed rays, 16 rows x 64 / 250 / 256 columns (250: a ragged last tile
column; the first column's Gaussians reach over the seam), lists of more than one 64-entry chunk, rays that cross one half, rays that
never do and pixels without a taker.  Every scene runs in four child processes -- LIDARGS_FUSED = 0 / 1 (the median launch sits behind
either form of the blend) x LIDARGS_TILE_ROWS = 4 / 32, which are read once per process -- started together; a fifth child does what
hangs on the buffers and the refusals.  LIDARGS_DEPTH itself is read at every forward and is set inside the children only.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import median_ref as mr
from util import (FLOOR, GRAD_KEYS_SR, RTOL, hip_forward_backward, oracle_backward_exact_sums, oracle_forward_backward, parity, parity_or_closer,
                  run_child)

pytestmark = pytest.mark.gpu

SWITCH = "LIDARGS_DEPTH"
H = mr.H
PLANS = {"fused_rows4": {"LIDARGS_FUSED": "1", "LIDARGS_TILE_ROWS": "4"}, "fused_rows32": {"LIDARGS_FUSED": "1", "LIDARGS_TILE_ROWS": "32"},
         "segmented_rows4": {"LIDARGS_FUSED": "0", "LIDARGS_TILE_ROWS": "4"}, "segmented_rows32": {"LIDARGS_FUSED": "0", "LIDARGS_TILE_ROWS": "32"}}
IMAGE_KEYS = ("color", "depth", "occ", "radii")
BUFFER_SCENE = "shell256"


def _with_switch(value, fn):
    if value is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = value
    try:
        return fn()
    finally:
        os.environ.pop(SWITCH, None)


def child_plan(refs, out):
    """One child process: every scene's forward + backward in both modes, with the reference's masked depth gradient and with none."""
    assert SWITCH not in os.environ
    up = np.load(refs)
    res = {}
    for name in mr.SCENES:
        scene, W = mr.scene(name)
        masked = (up[f"{name}.gc"], up[f"{name}.gd_masked"], up[f"{name}.go"])
        nodepth = (masked[0], np.zeros_like(masked[1]), masked[2])
        for mode, value in (("median", "median"), ("default", None)):
            r = _with_switch(value, lambda: hip_forward_backward(scene, W, H, masked))
            res.update({f"{name}.{mode}.{k}": r[k] for k in IMAGE_KEYS + GRAD_KEYS_SR})
            r = _with_switch(value, lambda: hip_forward_backward(scene, W, H, nodepth))
            res.update({f"{name}.{mode}0.{k}": r[k] for k in GRAD_KEYS_SR})
    np.savez(out, **res)
    print("OK")


class _Frame:
    """A forward through the binding (`_C`), keeping the opaque buffers at hand so that a backward can be run on them, on clones of
    them, or again (as tests/test_deterministic_gpu.py does)."""

    def __init__(self, name, grads):
        import torch
        from diff_lidargs_rasterization import _C
        from util import to_torch
        self.torch, self._C = torch, _C
        self.scene, self.W = mr.scene(name)
        self.st = to_torch(self.scene)
        self.grads = [torch.from_numpy(np.ascontiguousarray(g)).cuda() for g in grads]
        self.empty = torch.empty(0, device="cuda")

    def forward(self):
        st, e = self.st, self.empty
        return self._C.rasterize_gaussians(st["bg"], st["means3D"], st["colors"], st["opacities"], st["scales"], st["rotations"], 1.0, e,
                                           st["viewmatrix"], st["viewmatrix"], H, self.W, st["beams"], e, 1, e, False, 80, 0, False)

    def backward(self, fwd, clone=False):
        st, e = self.st, self.empty
        R, radii, geom, binning, img = fwd[0], fwd[4], fwd[5], fwd[6], fwd[7]
        if clone:
            radii, geom, binning, img = (t.clone() for t in (radii, geom, binning, img))
        g = self._C.rasterize_gaussians_backward(st["bg"], st["means3D"], radii, st["colors"], st["scales"], st["rotations"], 1.0, e,
                                                 st["viewmatrix"], st["viewmatrix"], st["beams"], 1.0, 1.0, *self.grads, e, 1, e,
                                                 geom, R, binning, img, False)
        return {k: g[i].cpu().numpy() for k, i in (("dL_dmeans2D", 0), ("dL_dcolors", 1), ("dL_dopacity", 2), ("dL_dmeans3D", 3), ("dL_dscales", 6),
                                                   ("dL_drotations", 7))}


def _surfel_forward():
    from util import hip_surfel_forward_backward, surfel_scene
    return hip_surfel_forward_backward(surfel_scene("street", 2000, 16, 93), 256, 16)["color"]


def _sharded_forward(cls):
    import torch
    import lidargs_dist
    import lidargs_scenes as sc
    from util import make_settings, to_torch
    st = to_torch(sc.make_scene("shell", 2000, 16, 94, random_view=True))
    mod = cls(make_settings(st, 256, 16), lidargs_dist.SingleComm())
    means2D = torch.zeros((2000, 4), device="cuda")
    return mod(st["means3D"], means2D, st["opacities"], st["colors"], st["scales"], st["rotations"])[0].cpu().numpy()


def _shell_forward():
    import lidargs_dist
    return _sharded_forward(lidargs_dist.ShellRasterizer)


def _wedge_forward():
    import lidargs_dist
    return _sharded_forward(lidargs_dist.WedgeRasterizer)


def _enqueue_only_forward():
    """Two frames: the module's first frame is an ordinary lidargs_forward that teaches it its capacity, the second is enqueue-only.
    The switch is set for the second only."""
    import torch
    import lidargs_scenes as sc
    from diff_lidargs_rasterization import GaussianRasterizer
    from util import make_settings, to_torch
    st = to_torch(sc.make_scene("street", 2000, 16, 95, random_view=True))
    rast = GaussianRasterizer(make_settings(st, 256, 16))
    rast.enqueue_only = True
    want = os.environ.pop(SWITCH, None)
    out = None
    for i in range(2):
        if i == 1 and want is not None:
            os.environ[SWITCH] = want
        out = rast(means3D=st["means3D"], means2D=torch.zeros((2000, 4), device="cuda"), opacities=st["opacities"], colors_precomp=st["colors"],
                   scales=st["scales"], rotations=st["rotations"])
    assert rast._enqueue.frames == 1
    return out[0].cpu().numpy()


def _deterministic_and_median():
    scene, W = mr.scene("shell64")
    os.environ["LIDARGS_DETERMINISTIC"] = "1"
    try:
        return hip_forward_backward(scene, W, H)["color"]
    finally:
        del os.environ["LIDARGS_DETERMINISTIC"]


REFUSING = {"surfel": _surfel_forward, "shell_world_of_one": _shell_forward, "wedge_world_of_one": _wedge_forward,
            "enqueue_only": _enqueue_only_forward, "deterministic_and_median": _deterministic_and_median}


def child_buffers(refs, out):
    """The fifth child: buffer sizes, the id plane, backward twice / on clones with the variable unset, a default forward's backward in
    a process that has made median buffers, the values of the switch, and the refusals."""
    assert SWITCH not in os.environ
    up = np.load(refs)
    name = BUFFER_SCENE
    fr = _Frame(name, (up[f"{name}.gc"], up[f"{name}.gd_masked"], up[f"{name}.go"]))
    res = {}
    sizes = lambda fwd: np.array([int(t.numel()) for t in fwd[5:8]], np.int64)
    plain = fr.forward()
    res["sizes_never_set"] = sizes(plain)
    res["never_set.depth"] = plain[2].cpu().numpy()
    before = fr.backward(plain)                                   # (no median forward yet in this process: today's launches)
    res.update({f"before.{k}": v for k, v in before.items()})
    for value in ("", "Median", "1", "expected"):
        res[f"sizes[{value}]"] = _with_switch(value, lambda: sizes(fr.forward()))
    on = _with_switch("median", fr.forward)
    res["sizes_switch_on"] = sizes(on)
    res["median.depth"] = on[2].cpu().numpy()
    n_img = int(res["sizes_never_set"][2])
    off = (n_img - 128 + 127) // 128 * 128                        # (lidargs_common.h img_carve: the plane starts at the next 128-byte boundary)
    res["median_id"] = on[7][off:off + 4 * H * fr.W].cpu().numpy().view(np.uint32).reshape(H, fr.W)
    # the variable is unset from here on: the mode travels in the buffers
    for what, fn in (("first", lambda: fr.backward(on)), ("second", lambda: fr.backward(on)), ("cloned", lambda: fr.backward(on, clone=True))):
        res.update({f"{what}.{k}": v for k, v in fn().items()})
    off_again = fr.forward()                                      # a default forward in a process that has made median buffers
    res["sizes_set_and_unset"] = sizes(off_again)
    res.update({f"default_after.{k}": v for k, v in fr.backward(off_again).items()})
    res.update({f"default_after_cloned.{k}": v for k, v in fr.backward(off_again, clone=True).items()})
    res.update({f"third.{k}": v for k, v in fr.backward(on).items()})     # ... and the median buffers again behind it
    for case, forward in REFUSING.items():
        ok_before = bool(np.isfinite(_with_switch(None, forward)).all()) if case != "deterministic_and_median" else True
        try:
            _with_switch("median", forward)
            msg = "no error"
        except RuntimeError as e:
            msg = "RuntimeError: " + str(e)
        ok_after = bool(np.isfinite(_with_switch(None, forward)).all())
        res[f"refusal.{case}"] = np.array([msg, str(ok_before), str(ok_after)])
    np.savez(out, **res)
    print("OK")


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """Per scene: the restatement and the float64 reference gradients for upstream gradients whose depth part is masked on undecided
    pixels (median_ref.reference), and the CPU oracle's default-mode backward for the same upstream gradients without a depth part,
    with its exact sums.  Computed once; the upstream gradients go to the children in a file."""
    out, up = {}, {}
    for name in mr.SCENES:
        scene, W = mr.scene(name)
        gc, gd, go = mr.upstream(name)
        ref = mr.reference(scene, W, H, (gc, gd, go))
        nodepth = (gc, np.zeros_like(gd), go)
        ora = oracle_forward_backward(scene, W, H, nodepth)
        ora64 = oracle_backward_exact_sums(ora, nodepth)
        ref0 = mr.reference(scene, W, H, nodepth, f=ref["fwd"]) if name in mr.BACKWARD_SCENES else None
        out[name] = dict(scene=scene, W=W, ref=ref, ref0=ref0, oracle0=ora, oracle0_64=ora64)
        up.update({f"{name}.gc": gc, f"{name}.gd_masked": ref["dL_ddepth_masked"], f"{name}.go": go})
    path = str(tmp_path_factory.mktemp("median") / "upstream.npz")
    np.savez(path, **up)
    out["path"] = path
    return out


@pytest.fixture(scope="module")
def runs(hip_lib_built, refs, tmp_path_factory):
    """{plan: arrays of child_plan} and {"buffers": arrays of child_buffers}, the five children running side by side."""
    d = tmp_path_factory.mktemp("median_runs")
    code = "import os\nos.environ.pop(%r, None)\nimport test_median_depth_gpu as t\nt.%s(sys.argv[1], sys.argv[2])"
    jobs = {plan: (code % (SWITCH, "child_plan"), env) for plan, env in PLANS.items()}
    jobs["buffers"] = (code % (SWITCH, "child_buffers"), {})
    outs = {k: str(d / f"{k}.npz") for k in jobs}
    with ThreadPoolExecutor(len(jobs)) as pool:
        fut = [pool.submit(run_child, body, env, (refs["path"], outs[k]), 300) for k, (body, env) in jobs.items()]
        for f in fut:
            f.result()
    return {k: dict(np.load(o)) for k, o in outs.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


@pytest.mark.parametrize("name", mr.SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_forward_returns_the_median_range(plan, name, runs, refs):
    """On every decided pixel the range of the restatement's Gaussian comes back (a wrong neighbour differs by metres, which no
    tolerance hides: every decided pixel is held to the parity metric's bar, none is a `flip`), 0 where no pixel takes anything;
    colour, occupancy and radii are the same child's default forward, bit for bit."""
    r, ref = runs[plan], refs[name]["ref"]
    got, dec = r[f"{name}.median.depth"][0], ref["decided"]
    want = ref["median_depth"]
    assert dec.sum() >= 0.98 * ref["has_taker"].sum()
    st = parity(f"{plan}.{name}.median depth", got[dec], want[dec])
    err = np.abs(got[dec] - want[dec]) / (np.abs(want[dec]) + FLOOR * np.abs(want[dec]).max())
    print(f"decided pixels: {int(dec.sum())} of {dec.size}, worst error {err.max():.2e}, wrong Gaussians: {int((err > 1e-3).sum())}")
    assert err.max() <= RTOL, f"{int((err > RTOL).sum())} decided pixels return another range than the restatement's Gaussian's"
    assert (got[~ref["has_taker"] & dec] == 0).all()
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
    r, ref, ref0 = runs[plan], refs[name]["ref"], refs[name]["ref0"]
    over = lambda got, want: int((np.abs(got - want) / (np.abs(want) + FLOOR * np.abs(want).max() + 1e-30) > RTOL).sum())
    failed = []
    for k in GRAD_KEYS_SR:
        try:
            parity(f"{plan}.{name}.{k}", r[f"{name}.median.{k}"], ref[k])
        except AssertionError as e:
            # where the budget is missed: the same count for the default mode's backward of the same child without a depth gradient
            # (no code of the median mode runs there) and for the float32 CPU oracle, each against its own float64 reference
            failed.append(f"{e} [entries over {RTOL:g}: median mode {over(r[f'{name}.median.{k}'], ref[k])}, default mode without a depth "
                          f"gradient {over(r[f'{name}.default0.{k}'], ref0[k])}, CPU oracle {over(refs[name]['oracle0'][k], ref0[k])}]")
    assert not failed, failed


@pytest.mark.parametrize("name", mr.SCENES)
@pytest.mark.parametrize("plan", list(PLANS))
def test_without_a_depth_gradient_the_backward_is_the_default_modes(plan, name, runs, refs):
    """dL/ddepth = 0: the blend's depth terms and the median add both vanish, and the gradients are the default mode's on the same scene
    within the backward's own run-to-run band (float atomics in scheduling order)."""
    r = runs[plan]
    for k in GRAD_KEYS_SR:
        parity_or_closer(f"{plan}.{name}.{k} (no depth gradient)", r[f"{name}.median0.{k}"], r[f"{name}.default0.{k}"], refs[name]["oracle0_64"][k])


def test_depth_gradient_lands_on_exactly_one_gaussian(runs, refs):
    """median - median0 is the depth part alone: dL/dmeans3D rows differ exactly for the Gaussians that are some decided pixel's median
    with a non-zero upstream gradient (one Gaussian per pixel), and colours / opacities carry none of it."""
    for plan in PLANS:
        for name in mr.RANDOM:
            r, ref = runs[plan], refs[name]["ref"]
            gd = ref["dL_ddepth_masked"][0]
            ok = (ref["median_id"] >= 0) & (gd != 0)
            want = np.zeros(ref["dL_dmeans3D"].shape[0])
            np.add.at(want, ref["median_id"][ok], gd[ok].astype(np.float64))
            moved = np.abs(r[f"{name}.median.dL_dmeans3D"].astype(np.float64) - r[f"{name}.median0.dL_dmeans3D"]).max(1)
            scale = np.abs(r[f"{name}.median0.dL_dmeans3D"]).max(1) + np.abs(want)
            assert not (moved[want == 0] > 1e-3 * (scale[want == 0] + 1e-6)).any(), (plan, name)
            big = np.abs(want) > 1e-2 * np.abs(want).max()
            assert (moved[big] > 0).all() and big.sum() >= 20, (plan, name)
            got_norm = np.linalg.norm(r[f"{name}.median.dL_dmeans3D"].astype(np.float64) - r[f"{name}.median0.dL_dmeans3D"], axis=1)
            np.testing.assert_allclose(got_norm[big], np.abs(want[big]), rtol=2e-2)      # |d range / d mean| = 1 (differences of float32 sums)
            for k in ("dL_dcolors", "dL_dopacity"):
                parity_or_closer(f"{plan}.{name}.{k} (depth part)", r[f"{name}.median.{k}"], r[f"{name}.median0.{k}"], refs[name]["oracle0_64"][k])


def test_buffer_sizes_and_values_of_the_switch(runs):
    """Only the image buffer grows, by the id plane (4 B per pixel, plus alignment); unset, empty and any value but the literal `median`
    ask for today's sizes -- also after the mode has been used in the process."""
    b = runs["buffers"]
    extra = b["sizes_switch_on"] - b["sizes_never_set"]
    N = H * mr.RANDOM[BUFFER_SCENE][2]
    assert extra[0] == 0 and extra[1] == 0 and 4 * N <= extra[2] <= 4 * N + 256, extra
    for value in ("", "Median", "1", "expected"):
        assert (b[f"sizes[{value}]"] == b["sizes_never_set"]).all(), value
    assert (b["sizes_set_and_unset"] == b["sizes_never_set"]).all()


def test_the_id_plane_names_the_restatements_gaussian(runs, refs):
    b, ref = runs["buffers"], refs[BUFFER_SCENE]["ref"]
    ids = b["median_id"].astype(np.int64)
    ids[ids == 0xFFFFFFFF] = -1
    dec = ref["decided"]
    assert dec.sum() >= 0.98 * ref["has_taker"].sum() and (ref["median_id"] >= 0).sum() > 1000
    wrong = int((ids[dec] != ref["median_id"][dec]).sum())
    print(f"decided pixels {int(dec.sum())}, other Gaussian than the restatement's: {wrong}")
    assert wrong == 0
    assert not same_bits(b["median.depth"], b["never_set.depth"])


def test_backward_twice_and_on_cloned_buffers_with_the_variable_unset(runs, refs):
    """The mode travels in the buffers: forward under the switch, variable removed, then backward, backward again (retain_graph) and
    backward on clones of every saved tensor -- all three the reference's gradients, and each other's within the run-to-run band."""
    b, ref = runs["buffers"], refs[BUFFER_SCENE]["ref"]
    for k in GRAD_KEYS_SR:
        for what in ("first", "second", "cloned", "third"):
            parity(f"buffers.{what}.{k}", b[f"{what}.{k}"], ref[k], verbose=False)
        for what in ("second", "cloned", "third"):
            parity(f"buffers.{what} against first.{k}", b[f"{what}.{k}"], b[f"first.{k}"], verbose=False)
    assert np.abs(b["first.dL_dmeans3D"] - b["before.dL_dmeans3D"]).max() > 1e-2 * np.abs(b["first.dL_dmeans3D"]).max()   # (the modes do differ)


def test_a_default_buffer_gets_the_default_gradients_after_a_median_forward(runs, refs):
    """The buffer's mode bit decides, not the process: a default forward's backward after the process has made median buffers (its
    backward now asks the mode word and queues the median add, which must retire) is the default backward of before -- the CPU oracle's
    gradients for the same upstream gradients, depth part included."""
    import lidargs_scenes as sc  # noqa: F401
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
    """The surfel variant (it has a median plane of its own), shells and wedges, the enqueue-only forward, and lidargs_forward under
    LIDARGS_DETERMINISTIC=1 as well: a RuntimeError naming the variable.  Without the switch they run, before and after."""
    msg, ok_before, ok_after = runs["buffers"][f"refusal.{case}"]
    assert msg.startswith("RuntimeError") and SWITCH in msg, msg
    assert ok_before == "True" and ok_after == "True"
