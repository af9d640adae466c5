"""LIDARGS_DETERMINISTIC=1: bit-reproducible gradients from the 3-D rasterizer (DESIGN.md "Deterministic backward").

In the default mode every (patch, segment) workgroup of the backward blend adds an entry's sixteen wave-reduced sums to the Gaussian's
gradient line with float atomics, so the rounding depends on which workgroup arrives first.  Under the switch `lidargs_forward` makes
buffers on which every `lidargs_backward` is a pure function of its inputs: not of the workgroups' order (work list against slot grid),
not of what ran before, not of a second backward on the same buffers -- and not of the environment at the time of the backward, since
the mode travels in the geometry buffer.

Scenes: 32 x 512 pixels, 4096 Gaussians, opacities U(0.05, 1), a scale modifier that spreads a footprint over several 16 x 4 patches.
How many Gaussians' lines receive terms from at least three workgroups, counted with the CPU oracle as the Gaussians that contribute
(dL/dopacity != 0 for upstream gradients masked to the patch) in at least three different 16 x 4 patches -- a lower bound, a patch's list
being walked by one workgroup per 64-entry segment:
    street  (scale modifier 4)   3007 Gaussians touched,  1626 in >= 2 patches,  764 in >= 3,  150 in >= 8  (most: 40 patches)
    shell   (scale modifier 3)   2039 Gaussians touched,  1713 in >= 2 patches,  957 in >= 3,  250 in >= 8  (most: 46 patches)
The shell scene runs with the segment plan forced to its shortest (LIDARGS_SEG_LEN=64), the street scene with the plan the library picks.

The plan switches (LIDARGS_WORK_LISTS, LIDARGS_FUSED, LIDARGS_SEG_LEN) are read once per process, so the launch-order comparison runs in
four child processes (two scenes x {work list, slot grid}), started together; LIDARGS_DETERMINISTIC itself is read at every forward and
is flipped inside one process everywhere else.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import lidargs_scenes as sc
from util import GRAD_KEYS_SR, hip_forward_backward, oracle_forward_backward, parity, run_child

pytestmark = pytest.mark.gpu

SWITCH = "LIDARGS_DETERMINISTIC"
P, H, W = 4096, 32, 512
SCENES = {
    # name: (kind, seed, scale modifier, plan switches of the child processes)
    "street": ("street", 91, 4.0, {"LIDARGS_FUSED": "0"}),
    "shell": ("shell", 92, 3.0, {"LIDARGS_FUSED": "0", "LIDARGS_SEG_LEN": "64"}),
}
IMAGE_KEYS = ("color", "depth", "occ", "radii")
DET_RUNS, DEFAULT_RUNS = 3, 2


def make_scene(name):
    kind, seed, mod, _ = SCENES[name]
    scene = sc.make_scene(kind, P, H, seed, random_view=True)
    scene["opacities"] = np.random.default_rng([seed, 0xDE7]).uniform(0.05, 1.0, (P, 1)).astype(np.float32)
    return scene, sc.upstream_grads(H, W, seed), mod


def same_bits(a, b):
    """Equal bit for bit (so NaN positions and the sign of a zero count too)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def _buffer_sizes(scene, mod):
    """What the three allocator callbacks are asked for by one forward (the opaque tensors are exactly that long)."""
    import torch
    from diff_lidargs_rasterization import _C
    from util import to_torch
    st = to_torch(scene)
    empty = torch.empty(0, device="cuda")
    fwd = _C.rasterize_gaussians(st["bg"], st["means3D"], st["colors"], st["opacities"], st["scales"], st["rotations"], mod, empty,
                                 st["viewmatrix"], st["viewmatrix"], H, W, st["beams"], empty, 1, empty, False, 80, 0, False)
    return np.array([int(t.numel()) for t in fwd[5:8]], np.int64)


def child_main(name, out):
    """One child process: the scene's forward + backward DET_RUNS times under the switch and DEFAULT_RUNS times without, and the
    buffer sizes before the variable was ever set and after it was set and removed again."""
    assert SWITCH not in os.environ
    scene, grads, mod = make_scene(name)
    res = {"sizes_never_set": _buffer_sizes(scene, mod)}
    os.environ[SWITCH] = "1"
    res["sizes_switch_on"] = _buffer_sizes(scene, mod)
    for i in range(DET_RUNS):
        r = hip_forward_backward(scene, W, H, grads, scale_modifier=mod)
        res.update({f"det{i}.{k}": r[k] for k in IMAGE_KEYS + GRAD_KEYS_SR})
    del os.environ[SWITCH]
    res["sizes_set_and_unset"] = _buffer_sizes(scene, mod)
    for i in range(DEFAULT_RUNS):
        r = hip_forward_backward(scene, W, H, grads, scale_modifier=mod)
        res.update({f"default{i}.{k}": r[k] for k in IMAGE_KEYS + GRAD_KEYS_SR})
    np.savez(out, **res)
    print("OK")


@pytest.fixture(scope="module")
def runs(hip_lib_built, tmp_path_factory):
    """{(scene, "lists" | "grid"): arrays of child_main}, the four children running side by side."""
    code = f"import os\nos.environ.pop({SWITCH!r}, None)\nimport test_deterministic_gpu as t\nt.child_main(sys.argv[1], sys.argv[2])"
    d = tmp_path_factory.mktemp("deterministic")
    outs = {(name, order): str(d / f"{name}_{order}.npz") for name in SCENES for order in ("lists", "grid")}
    with ThreadPoolExecutor(len(outs)) as pool:
        runs = [pool.submit(run_child, code, dict(SCENES[name][3], LIDARGS_WORK_LISTS="1" if order == "lists" else "0"), (name, out), 300)
                for (name, order), out in outs.items()]
        for r in runs:
            r.result()
    return {key: dict(np.load(out)) for key, out in outs.items()}


@pytest.mark.parametrize("name", list(SCENES))
def test_gradients_are_bit_identical_whatever_the_launch_order(name, runs):
    """Work list against slot grid (the same (patch, segment) walks launched in very different orders), three times each in one
    process: every gradient array is equal bit for bit.  The same comparison in the default mode must differ somewhere -- if it does
    not, the scene does not exercise the order and has to be made harder."""
    lists, grid = runs[name, "lists"], runs[name, "grid"]
    for k in GRAD_KEYS_SR:
        first = lists[f"det0.{k}"]
        assert np.abs(first).max() > 0, k
        for i in range(DET_RUNS):
            assert same_bits(lists[f"det{i}.{k}"], first), (k, "work list, run", i)
            assert same_bits(grid[f"det{i}.{k}"], first), (k, "slot grid, run", i)
    default = [r[f"default{i}.{k}"] for r in (lists, grid) for i in range(DEFAULT_RUNS) for k in GRAD_KEYS_SR]
    n = len(GRAD_KEYS_SR)
    differs = [k for j, k in enumerate(GRAD_KEYS_SR) if any(not same_bits(default[j], default[m * n + j]) for m in range(1, 2 * DEFAULT_RUNS))]
    print("default mode differs from run to run in:", differs)
    assert differs, "float atomics gave the same bits in every order: the scene is too easy"


@pytest.mark.parametrize("name", list(SCENES))
def test_deterministic_gradients_match_the_oracle(name, runs):
    """The values: the default mode's parity budget against the CPU oracle, no new tolerance."""
    scene, grads, mod = make_scene(name)
    ref = oracle_forward_backward(scene, W, H, grads, scale_modifier=mod)
    for order in ("lists", "grid"):
        r = runs[name, order]
        mism = int((r["det0.radii"] != ref["radii"]).sum())
        assert mism <= 1, mism
        for k in ("color", "depth", "occ") + GRAD_KEYS_SR:
            parity(f"{name}.{order}.{k}", r[f"det0.{k}"], ref[k])


@pytest.mark.parametrize("name", list(SCENES))
def test_forward_and_default_buffers_are_unchanged(name, runs):
    """The forward has no float atomics: its outputs under the switch are the default mode's, bit for bit.  With the switch off the
    three allocators are asked for the same sizes in a process that never set the variable and in one that set and removed it; with
    it on only the geometry buffer grows, by the 64-bit lines (16 x 8 B per Gaussian, plus alignment)."""
    for order in ("lists", "grid"):
        r = runs[name, order]
        for k in IMAGE_KEYS:
            for i in range(DET_RUNS):
                assert same_bits(r[f"det{i}.{k}"], r[f"default0.{k}"]), (order, k, i)
        assert (r["sizes_never_set"] == r["sizes_set_and_unset"]).all(), (r["sizes_never_set"], r["sizes_set_and_unset"])
        extra = r["sizes_switch_on"] - r["sizes_never_set"]
        assert 128 * P <= extra[0] <= 128 * P + 256 and extra[1] == 0 and extra[2] == 0, extra
    assert (runs[name, "lists"]["sizes_never_set"][[0, 2]] == runs[name, "grid"]["sizes_never_set"][[0, 2]]).all()


class _Frame:
    """A forward through the binding (`_C`), keeping the opaque buffers at hand so that a backward can be run on them, on clones of
    them, or again."""

    def __init__(self, name):
        import torch
        from diff_lidargs_rasterization import _C
        from util import to_torch
        self.torch, self._C = torch, _C
        scene, grads, self.mod = make_scene(name)
        self.scene, self.grads_np = scene, grads
        self.st = to_torch(scene)
        self.grads = [torch.from_numpy(g).cuda() for g in grads]
        self.empty = torch.empty(0, device="cuda")

    def forward(self):
        st, e = self.st, self.empty
        return self._C.rasterize_gaussians(st["bg"], st["means3D"], st["colors"], st["opacities"], st["scales"], st["rotations"], self.mod, e,
                                           st["viewmatrix"], st["viewmatrix"], H, W, st["beams"], e, 1, e, False, 80, 0, False)

    def backward(self, fwd, clone=False):
        st, e = self.st, self.empty
        R, radii, geom, binning, img = fwd[0], fwd[4], fwd[5], fwd[6], fwd[7]
        if clone:
            radii, geom, binning, img = (t.clone() for t in (radii, geom, binning, img))
        g = self._C.rasterize_gaussians_backward(st["bg"], st["means3D"], radii, st["colors"], st["scales"], st["rotations"], self.mod, e,
                                                 st["viewmatrix"], st["viewmatrix"], st["beams"], 1.0, 1.0, *self.grads, e, 1, e,
                                                 geom, R, binning, img, False)
        # dL_dmeans2D (densification norm slot included), colors, opacity, means3D, cov3D, scales, rotations
        return {k: g[i].cpu().numpy() for k, i in (("dL_dmeans2D", 0), ("dL_dcolors", 1), ("dL_dopacity", 2), ("dL_dmeans3D", 3), ("dL_dcov3D", 4),
                                                   ("dL_dscales", 6), ("dL_drotations", 7))}


def _assert_same(got, want, what):
    for k in want:
        assert same_bits(got[k], want[k]), (what, k)


def test_backward_twice_and_on_cloned_buffers(hip_lib_built, monkeypatch):
    """retain_graph (a second backward on the same buffers must start from cleared accumulators, the 64-bit ones included), another
    frame's forward and backward in between, and a backward on clones of every saved tensor: bit-identical to the first backward."""
    monkeypatch.setenv(SWITCH, "1")
    fr = _Frame("street")
    fwd = fr.forward()
    first = fr.backward(fwd)
    assert np.abs(first["dL_dopacity"]).max() > 0 and np.abs(first["dL_dcov3D"]).max() > 0
    _assert_same(fr.backward(fwd), first, "second backward")
    other = _Frame("shell")
    other.backward(other.forward())
    _assert_same(fr.backward(fwd, clone=True), first, "cloned buffers, after another frame")
    _assert_same(fr.backward(fwd), first, "third backward")
    _assert_same(fr.backward(fr.forward()), first, "a second forward's backward")


def test_the_mode_travels_with_the_buffers(hip_lib_built, monkeypatch):
    """The forward decides, the backward reads no environment.  Forward under the switch, variable removed, backward: the
    deterministic result.  Forward without, variable set, backward: today's path -- today's buffer sizes, the oracle's values."""
    fr = _Frame("street")
    monkeypatch.setenv(SWITCH, "1")
    on = fr.forward()
    want = fr.backward(on)
    monkeypatch.delenv(SWITCH)
    _assert_same(fr.backward(on), want, "forward under the switch, backward without")
    _assert_same(fr.backward(on, clone=True), want, "... on cloned buffers")
    off = fr.forward()
    sizes_off = [int(t.numel()) for t in off[5:8]]
    assert off[0] == on[0] and sizes_off[1:] == [int(t.numel()) for t in on[6:8]] and sizes_off[0] < int(on[5].numel())
    monkeypatch.setenv(SWITCH, "1")
    got = fr.backward(off)                      # (128 * P bytes short of a deterministic buffer: the backward must not look behind it)
    monkeypatch.delenv(SWITCH)
    assert sizes_off == [int(t.numel()) for t in fr.forward()[5:8]]
    ref = oracle_forward_backward(fr.scene, W, H, fr.grads_np, scale_modifier=fr.mod)
    for k in GRAD_KEYS_SR:
        parity("default buffers, switch set at the backward: " + k, got[k], ref[k], verbose=False)
        parity("deterministic buffers, switch removed: " + k, want[k], ref[k], verbose=False)


def test_empty_and_values_of_the_switch(hip_lib_built, monkeypatch):
    """Unset, empty and 0 are the default path: the geometry buffer is not a byte longer."""
    fr = _Frame("street")
    monkeypatch.delenv(SWITCH, raising=False)
    plain = int(fr.forward()[5].numel())
    for v in ("", "0"):
        monkeypatch.setenv(SWITCH, v)
        assert int(fr.forward()[5].numel()) == plain, repr(v)
    monkeypatch.setenv(SWITCH, "1")
    assert int(fr.forward()[5].numel()) > plain


def _surfel_forward():
    from util import hip_surfel_forward_backward, surfel_scene
    return hip_surfel_forward_backward(surfel_scene("street", 2000, 16, 93), 256, 16)["color"]


def _sharded_forward(cls):
    import torch
    import lidargs_dist
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
    """Two frames: the module's first frame is an ordinary lidargs_forward that teaches it its capacity, the second is enqueue-only."""
    import torch
    from diff_lidargs_rasterization import GaussianRasterizer
    from util import make_settings, to_torch
    st = to_torch(sc.make_scene("street", 2000, 16, 95, random_view=True))
    rast = GaussianRasterizer(make_settings(st, 256, 16))
    rast.enqueue_only = True
    out = None
    for _ in range(2):
        out = rast(means3D=st["means3D"], means2D=torch.zeros((2000, 4), device="cuda"), opacities=st["opacities"], colors_precomp=st["colors"],
                   scales=st["scales"], rotations=st["rotations"])
    assert rast._enqueue.frames == 1
    return out[0].cpu().numpy()


@pytest.mark.parametrize("forward", [_surfel_forward, _shell_forward, _wedge_forward, _enqueue_only_forward],
                         ids=["surfel", "shell_world_of_one", "wedge_world_of_one", "enqueue_only"])
def test_entry_points_the_mode_does_not_cover_refuse_it(forward, hip_lib_built, monkeypatch):
    """A float-atomic backward under a switch that promises the opposite would be worse than an error: these forwards return
    LIDARGS_ERR_INVALID_ARGUMENT (a RuntimeError in the bindings) naming the switch.  Without it they run as before."""
    monkeypatch.delenv(SWITCH, raising=False)
    assert np.isfinite(forward()).all()
    monkeypatch.setenv(SWITCH, "1")
    with pytest.raises(RuntimeError, match=SWITCH):
        forward()
    monkeypatch.delenv(SWITCH)
    assert np.isfinite(forward()).all()
