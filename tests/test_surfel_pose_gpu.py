"""The surfel rasterizer's gradient with respect to the sensor pose (dL/dviewmatrix): the pose form of the per-surfel chain
(k_sf_gaussian_backward_view), the fold of its partial rows, `lgsfpose_backward_view` and the autograd plumbing of the surfel
`GaussianRasterizer`, against tests/surfel_pose_ref.py (itself held against float64 autograd by tests/test_surfel_pose_ref_cpu.py).

  (a) hook            `lgsfpose_debug_view_backward` on caller-supplied lines and marks against the float64 sum of the restatement's
                      per-surfel contributions, with its float32 run as the yardstick
  (b) end to end      `viewmatrix.requires_grad_()` through GaussianRasterizer against the restatement fed the oracle's blend sums, against
                      the restatement fed HIP's own dL_dtransMat / dL_dnormal, and the translation identity on HIP's own mean gradients
  (c) nothing moves   without the request the call is the one it was; with it the images keep their bits and the gradient rows stay
                      within the repeat spread of the blend's float atomics
  (d) other paths     the matrix as the only leaf, retain_graph, cloned buffers, no_grad, P = 0
  (e) refusals

The bar of (a), per entry k of the matrix, is the 3-D form's (tests/test_pose_gpu.py; the summation structure is identical):
|got - sum_i c64[i,k]| <= 4 sum_i |c32[i,k] - c64[i,k]| + 10 * 2^-24 sum_i |c64[i,k]|.  The first term is the project's factor 4 over an
independent float32 evaluation of every contribution; the second covers the kernel's own summation in float32 -- at most four adds per
lane and six levels of the wave's tree, ten roundings of relative size 2^-24 on partial sums bounded by sum |c| -- the fold of the
partial rows being in double.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import surfel_pose_ref
import surfel_ref as ref
from test_pose_gpu import _translation_identity
from test_preprocess_gpu import _ptr, _stream, _sync
from test_surfel_oracle_autograd_cpu import _close
from test_surfel_preprocess_gpu import ARRAYS, ROWS, Arr, Backward, chain_lines, reference
from util import oracle_surfel_forward_backward, surfel_scene, surfel_upstream_grads, to_torch

pytestmark = pytest.mark.gpu

USED = [4 * r + k for r in range(4) for k in range(3)]
COLUMN3 = [3, 7, 11, 15]
GRADS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dscales", "dL_drotations")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _sf():
    from diff_lidargs_surfel_rasterization import _C
    return _C


def partial_floats(P):
    n = int(_sf()._lib.lgsfpose_view_partial_floats(P))
    assert n == 16 * ((P + 255) // 256)
    return n


class ViewBackward(Backward):
    """The arrays of a lgsfpose_debug_view_backward call: test_surfel_preprocess_gpu.Backward's, the sixteen outputs and the partial rows
    (NaN before the call)."""

    def __init__(self, P, W, H, scene, radii, mod=1.0):
        super().__init__(P, W, H, scene, radii)
        self.mod = mod
        self.out = Arr.filled(16, np.float32)
        self.partials = Arr.filled(partial_floats(P), np.float32)

    def call_view(self, partial_floats_arg=None, **null):
        i = self.ins
        a = dict(gacc=self.gacc.ptr, means=_ptr(i.get("means")), view=_ptr(i.get("view")), out=self.out.ptr, partials=self.partials.ptr)
        a.update(null)
        n = self.partials.shape[0] if partial_floats_arg is None else partial_floats_arg
        rc = _sf()._lib.lgsfpose_debug_view_backward(self.P, self.W, self.H, a["gacc"], a["means"], _ptr(i.get("scales")), self.mod, _ptr(i.get("rots")),
                                                      a["view"], _ptr(i.get("beams")), _ptr(i.get("radii")), *[_ptr(self.rows[k]) for k, _ in ROWS],
                                                      self.depth.ptr, self.tlist.ptr, self.tcount.ptr, a["out"], a["partials"], n, _stream())
        _sync()
        return rc

    def run(self, line, marks):
        """lists and zeros (stage 1), the blend's fill, the pose form + fold -> (dL_dviewmatrix[16], partial rows, gradient rows + depth)."""
        self.touched.write(marks)
        assert self.call(1) == 0, _sf()._base._err()
        self.gacc.write(line)
        assert self.call_view() == 0, _sf()._base._err()
        self.gacc.read(); self.tlist.read(); self.tcount.read()
        rows = self.read_rows()
        rows["depth"] = self.depth.read()
        return self.out.read(), self.partials.read(), rows


def _marks(P, seed):
    """Region 0 whole (four trips of the 64-lane loop), region 1 empty where there are three regions or more, 40 % of the rest, the last
    surfel marked."""
    rng = np.random.default_rng([P, seed])
    marks = (rng.random(P) < 0.4).astype(np.uint8)
    marks[:256] = 1
    if P > 512:
        marks[256:512] = 0
    marks[P - 1] = 1
    return marks


@functools.lru_cache(maxsize=None)
def _hook_case(P):
    """(scene, W, H, radii, lines [P,32], marks): a street scene of P surfels under a random rigid view; every surfel counts as visible (the
    radii feed the depth plane alone).  Lines: test_surfel_preprocess_gpu.chain_lines -- the marked surfels carry random cotangents in the
    23 live slots and NaN in the dead ones, the unmarked surfels' lines are all NaN and must not be read."""
    W, H = 256, 32
    scene = surfel_scene("street", max(P, 512), H, 300 + P % 97, random_view=True)
    scene = {k: (np.ascontiguousarray(v[:P]) if k in ARRAYS else v) for k, v in scene.items()}
    marks = _marks(P, 77)
    return scene, W, H, np.ones(P, np.int32), chain_lines(P, marks != 0, 9), marks


def _bar(c64, c32):
    return 4.0 * np.abs(c32 - c64).sum(0) + 10.0 * 2.0 ** -24 * np.abs(c64).sum(0)


def _check_against_float64(what, got, scene, W, H, line, marks, mod=1.0):
    import torch
    fed = np.nan_to_num(line.astype(np.float64)) * (marks != 0)[:, None]
    args = (fed, scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], scene["beams"], W, H, mod)
    c64 = surfel_pose_ref.contributions(*args)
    c32 = surfel_pose_ref.contributions(*args, dtype=torch.float32)
    want, bar = c64.sum(0), _bar(c64, c32)
    err = np.abs(got.astype(np.float64) - want)
    for k in USED:
        print(f"[surfel pose {what}] vm[{k:2d}] got {got[k]: .7e}  float64 {want[k]: .7e}  |diff| {err[k]:.2e}  bar {bar[k]:.2e} "
              f"(fp32 yardstick {bar[k] - 10.0 * 2.0 ** -24 * np.abs(c64[:, k]).sum():.2e})")
    assert np.isfinite(got).all(), what
    assert np.abs(want[USED]).min() > 0, what
    for k in USED:
        assert err[k] <= bar[k], (what, k, err[k], bar[k])
    assert not got[COLUMN3].view(np.uint32).any(), what                     # read by no kernel: +0


def _hook(what, scene, W, H, radii, line, marks, mod=1.0):
    P = line.shape[0]
    b = ViewBackward(P, W, H, scene, radii, mod)
    got, partials, rows = b.run(line, marks)
    regions = (P + 255) // 256
    assert partials.size == 16 * regions and np.isfinite(partials).all()   # every region wrote its row over the NaNs; no NaN line was read
    part = partials.reshape(regions, 16)
    assert not part[:, COLUMN3].view(np.uint32).any()
    if P > 512:
        assert not part[1].view(np.uint32).any()                            # nothing touched: a row of +0
    _check_against_float64(what, got, scene, W, H, line, marks, mod)
    # the other outputs are the chain's, bit for bit
    plain = Backward(P, W, H, scene, radii)
    plain.touched.write(marks)
    assert plain.call(1) == 0
    plain.gacc.write(line)
    assert plain.call(2) == 0
    want_rows = plain.read_rows()
    want_rows["depth"] = plain.depth.read()
    assert set(want_rows) == set(rows)
    for k, a in want_rows.items():
        assert same_bits(a, rows[k]), k
    assert np.isfinite(rows["dL_dmean3D"]).all() and np.abs(rows["dL_dmean3D"][marks != 0]).max() > 0
    # and a second call on the same arrays gives the same sixteen floats and partial rows: no atomics on this path
    assert b.call_view() == 0
    assert same_bits(b.out.read(), got) and same_bits(b.partials.read(), partials)
    return got


@pytest.mark.parametrize("P", [1, 260, 1025, 70001])
def test_hook_against_float64(P, hip_lib_built):
    """One lane; a short last region; one region past a four-wave block; more partial rows (274) than the fold has row groups."""
    scene, W, H, radii, line, marks = _hook_case(P)
    _hook(f"P={P}", scene, W, H, radii, line, marks)


def test_hook_with_scale_modifier_6(hip_lib_built):
    """The modifier reaches the pose gradient (and no other output: the rows are compared with the plain chain's, which does not read it)."""
    scene, W, H, radii, line, marks = _hook_case(1025)
    got6 = _hook("mod=6", scene, W, H, radii, line, marks, mod=6.0)
    got1, _, _ = ViewBackward(1025, W, H, scene, radii, 1.0).run(line, marks)
    assert same_bits(got6[12:15], got1[12:15]) and not same_bits(got6[:12], got1[:12])       # the axes do not reach the translation row


def test_hook_on_the_seam_scene(hip_lib_built):
    """test_surfel_preprocess_gpu's scene 6 at W = 250: surfels on both sides of the panorama's seam, every seventh one a large disc."""
    d, f, geo, tk = reference("6_seam_W250")
    s = d["scene"]
    P = s["means3D"].shape[0]
    radii = np.where(geo["live"], np.maximum(geo["rx"], geo["ry"]), 0).astype(np.int32)
    marks = _marks(P, 78)
    _hook("seam W=250", s, d["W"], d["H"], radii, chain_lines(P, marks != 0, 10), marks)


# ---- (b) end to end -----------------------------------------------------------------------------------------------------------------
E2E = {"shell": (3000, 16, 512, 3), "street": (10_000, 16, 512, 1)}         # tests/test_surfel_gpu.py's small scenes at their image sizes


@functools.lru_cache(maxsize=None)
def _e2e_scene(kind):
    P, H, W, seed = E2E[kind]
    return surfel_scene(kind, P, H, seed), W, H, surfel_upstream_grads(H, W, seed)


def _settings(st, W, H, mod=1.0):
    import torch
    from diff_lidargs_surfel_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=int(H), image_width=int(W), bg=st["bg"], scale_modifier=mod, depth_threshold=0.0, viewmatrix=st["viewmatrix"],
        projmatrix=torch.eye(4, device="cuda"), sh_degree=1, campos=torch.zeros(3, device="cuda"), prefiltered=False,
        beam_inclinations=st["beams"], lidar_far=80, lidar_near=0, debug=False)


def _render(scene, W, H, grads, pose, only_pose=False, retain=False):
    """One forward + backward through the surfel GaussianRasterizer; pose: the matrix requires grad.  -> dict of numpy results (+ the
    live tensors)."""
    import torch
    from diff_lidargs_surfel_rasterization import GaussianRasterizer
    st = to_torch(scene)
    P = st["means3D"].shape[0]
    leaves = {k: st[k].clone().requires_grad_(not only_pose) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    means2D = torch.zeros((P, 4), dtype=torch.float32, device="cuda", requires_grad=not only_pose)
    vm = st["viewmatrix"].clone().requires_grad_(pose)
    rast = GaussianRasterizer(_settings(dict(st, viewmatrix=vm), W, H))
    color, radii, others, pixels = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=None,
                                        colors_precomp=leaves["colors"], scales=leaves["scales"], rotations=leaves["rotations"])
    g = [torch.from_numpy(x).cuda() for x in grads]
    torch.autograd.backward([color, others], g, retain_graph=retain)
    out = dict(color=color.detach().cpu().numpy(), others=others.detach().cpu().numpy(), radii=radii.cpu().numpy(), pixels=pixels.cpu().numpy())
    if not only_pose:
        out.update(dL_dmeans3D=leaves["means3D"].grad.cpu().numpy(), dL_dmeans2D=means2D.grad.cpu().numpy(), dL_dcolors=leaves["colors"].grad.cpu().numpy(),
                   dL_dopacity=leaves["opacities"].grad.cpu().numpy(), dL_dscales=leaves["scales"].grad.cpu().numpy(),
                   dL_drotations=leaves["rotations"].grad.cpu().numpy())
    out["dL_dviewmatrix"] = None if vm.grad is None else vm.grad.cpu().numpy()
    out["live"] = (vm, [color, others], g)
    return out


def _direct(scene, W, H, grads, clone_buffers=False, **kw):
    """The binding's two functions called directly -> (forward tuple, backward tuple)."""
    import torch
    C_ = _sf()
    st = to_torch(scene)
    e = torch.empty(0, device="cuda")
    eye, z3 = torch.eye(4, device="cuda"), torch.zeros(3, device="cuda")
    fwd = C_.rasterize_gaussians(st["bg"], st["means3D"], st["colors"], st["opacities"], st["scales"], st["rotations"], 1.0, e, st["viewmatrix"], eye,
                                 st["beams"], H, W, e, 1, z3, False, 80, 0, False)
    radii, geom, binning, img = (t.clone() if clone_buffers else t for t in (fwd[3], fwd[5], fwd[6], fwd[7]))
    g = [torch.from_numpy(x).cuda() for x in grads]
    bwd = C_.rasterize_gaussians_backward(st["bg"], st["means3D"], radii, st["colors"], st["scales"], st["rotations"], 1.0, e, st["viewmatrix"], eye,
                                          st["beams"], g[0], g[1], e, 1, z3, geom, fwd[0], binning, img, False, **kw)
    return fwd, bwd


@pytest.mark.parametrize("kind", ["shell", "street"])
def test_end_to_end_against_the_restatement(kind, hip_lib_built):
    scene, W, H, grads = _e2e_scene(kind)
    P = scene["means3D"].shape[0]
    r = _render(scene, W, H, grads, pose=True)
    gvm = r["dL_dviewmatrix"]
    assert gvm is not None and gvm.shape == (4, 4) and gvm.dtype == np.float32
    got = gvm.reshape(16)
    args = (scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], scene["beams"], W, H)
    # the restatement fed the oracle's line
    o = oracle_surfel_forward_backward(scene, W, H, grads)
    Tw = o["fwd"].array("transMat").reshape(P, 9)[:, 6:9].astype(np.float64)
    want = surfel_pose_ref.contributions(ref.line_from_oracle(o, Tw, scene["beams"], W, H), *args).sum(0)
    print(f"[surfel pose {kind}] got {got[USED]}\n[surfel pose {kind}] want {want[USED]}")
    assert not got[COLUMN3].view(np.uint32).any()
    _close(f"dL_dviewmatrix {kind}", got[USED], want[USED])
    _translation_identity(f"surfel {kind}", scene, gvm, r["dL_dmeans3D"])
    # the restatement fed HIP's own rows of one backward: dL_dtransMat (its third row is the final dL/dTw) and dL_dnormal, which shares
    # the returned rows' slab (the reference's torch::zeros list, R2/rasterize_points.cu:193-203: means3D, means2D, colors, normal, ...)
    import torch
    fwd, bwd = _direct(scene, W, H, grads, want_intermediates=True, want_viewmatrix_grad=True)
    assert len(bwd) == 10 and bwd[9].shape == (4, 4) and bwd[9].dtype == torch.float32
    slab = bwd[3]._base
    assert slab is not None and slab.numel() == 32 * P and bwd[3].data_ptr() == slab.data_ptr()
    gn = slab[P * 9:P * 12].view(P, 3).cpu().numpy()
    gT = bwd[4].cpu().numpy()
    line = np.zeros((P, 32), np.float32)
    for k, v in (("TU", gT[:, 0:3]), ("TV", gT[:, 3:6]), ("TW", gT[:, 6:9]), ("N", gn)):
        line[:, list(ref.SLOT[k])] = v
    assert np.abs(gn).max() > 0 and np.abs(gT).max() > 0
    c64 = surfel_pose_ref.contributions(line, *args)
    c32 = surfel_pose_ref.contributions(line, *args, dtype=torch.float32)
    own = bwd[9].cpu().numpy().reshape(16)
    err, bar = np.abs(own.astype(np.float64) - c64.sum(0)), _bar(c64, c32)
    for k in USED:
        print(f"[surfel pose {kind}, own rows] vm[{k:2d}] got {own[k]: .7e}  float64 {c64[:, k].sum(): .7e}  |diff| {err[k]:.2e}  bar {bar[k]:.2e}")
    for k in USED:
        assert err[k] <= bar[k], (kind, k, err[k], bar[k])
    _translation_identity(f"surfel {kind}, direct", scene, bwd[9].cpu().numpy(), bwd[3].cpu().numpy())


# ---- (c) what must not move ---------------------------------------------------------------------------------------------------------
def test_nothing_moves_without_the_request_and_little_with_it(hip_lib_built, monkeypatch):
    """The surfel blend's backward adds with float atomics and has no deterministic mode, so a frame does not repeat its own gradient
    bits: the no-request frame run twice gives the spread, and the frame with the request stays within twice that, per array."""
    C_ = _sf()
    scene, W, H, grads = _e2e_scene("street")
    calls = []
    real = C_.rasterize_gaussians_backward
    monkeypatch.setattr(C_, "rasterize_gaussians_backward", lambda *a, **kw: calls.append((kw, real(*a, **kw))) or calls[-1][1])
    off = _render(scene, W, H, grads, pose=False)
    assert off["dL_dviewmatrix"] is None
    assert list(calls[0][0]) == ["want_intermediates"] and calls[0][0]["want_intermediates"] is False and len(calls[0][1]) == 9    # the call it always was
    off2 = _render(scene, W, H, grads, pose=False)
    on = _render(scene, W, H, grads, pose=True)
    assert calls[2][0].get("want_viewmatrix_grad") is True and len(calls[2][1]) == 10
    monkeypatch.setattr(C_, "rasterize_gaussians_backward", real)
    for k in ("color", "others", "radii", "pixels"):
        assert same_bits(off[k], off2[k]) and same_bits(on[k], off[k]), k
    for k in GRADS:
        spread = float(np.abs(off[k].astype(np.float64) - off2[k]).max())
        moved = float(np.abs(on[k].astype(np.float64) - off[k]).max())
        print(f"[surfel pose] {k}: repeat spread {spread:.3e}, with the request {moved:.3e}, max |x| {np.abs(off[k]).max():.3e}")
        assert np.abs(off[k]).max() > 0
        assert moved <= 2.0 * spread, k
    assert np.abs(on["dL_dviewmatrix"].reshape(16)[USED]).min() > 0


# ---- (d) other paths ----------------------------------------------------------------------------------------------------------------
def _same_sum(what, a, b):
    """Two evaluations of one frame's gradient on lines whose float atomics ran in another order: the 3-D form's bar for the same
    comparison (tests/test_pose_gpu.py test_the_matrix_as_the_only_leaf), 1e-5 of each entry with a floor of 1e-3 of the largest."""
    _close(what, a.reshape(16)[USED], b.reshape(16)[USED], rtol=1e-5, worst=1e-5)


def test_the_matrix_as_the_only_leaf_and_retain_graph(hip_lib_built):
    import torch
    scene, W, H, grads = _e2e_scene("shell")
    full = _render(scene, W, H, grads, pose=True)["dL_dviewmatrix"]
    r = _render(scene, W, H, grads, pose=True, only_pose=True, retain=True)
    assert r["dL_dviewmatrix"] is not None and "dL_dmeans3D" not in r
    _same_sum("only leaf", r["dL_dviewmatrix"], full)
    vm, outs, g = r["live"]
    vm.grad = None
    torch.autograd.backward(outs, g)                                        # retain_graph: the same forward's buffers once more
    _same_sum("retain_graph", vm.grad.cpu().numpy(), full)


def test_backward_on_cloned_buffers(hip_lib_built):
    scene, W, H, grads = _e2e_scene("shell")
    full = _render(scene, W, H, grads, pose=True)["dL_dviewmatrix"]
    _, bwd = _direct(scene, W, H, grads, clone_buffers=True, want_intermediates=False, want_viewmatrix_grad=True)
    assert bwd[4] is None and len(bwd) == 10
    _same_sum("cloned buffers", bwd[9].cpu().numpy(), full)


def test_no_grad_requests_nothing_and_an_empty_frame_gives_zeros(hip_lib_built, monkeypatch):
    import torch
    import diff_lidargs_surfel_rasterization as pkg
    scene, W, H, grads = _e2e_scene("shell")
    st = to_torch(scene)
    vm = st["viewmatrix"].clone().requires_grad_(True)
    rast = pkg.GaussianRasterizer(_settings(dict(st, viewmatrix=vm), W, H))
    used = []                                                               # the pose node's forward (and the request itself) pass through here
    real = pkg._C.refuse_pose_with_transmat
    monkeypatch.setattr(pkg._C, "refuse_pose_with_transmat", lambda tm: used.append(1) or real(tm))
    call = lambda n: rast(means3D=st["means3D"][:n], means2D=torch.zeros((n, 4), device="cuda"), opacities=st["opacities"][:n], shs=None,
                          colors_precomp=st["colors"][:n], scales=st["scales"][:n], rotations=st["rotations"][:n])
    with torch.no_grad():
        color, _, others, _ = call(100)
    assert not used and not color.requires_grad and not others.requires_grad
    color, _, others, _ = call(0)                                           # P = 0: a node, a backward, sixteen zeros
    assert used and color.requires_grad
    torch.autograd.backward([color, others], [torch.from_numpy(x).cuda() for x in grads])
    assert vm.grad.shape == (4, 4) and vm.grad.dtype == torch.float32 and not vm.grad.cpu().numpy().view(np.uint32).any()


# ---- (e) refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib_built):
    import torch
    import diff_lidargs_surfel_rasterization as pkg
    # a precomputed transform together with the request: a RuntimeError from the node's forward, naming both
    scene, W, H, grads = _e2e_scene("shell")
    st = to_torch(scene)
    n = 64
    vm = st["viewmatrix"].clone().requires_grad_(True)
    args = (st["means3D"][:n], torch.zeros((n, 4), device="cuda"), torch.empty(0, device="cuda"), st["colors"][:n], st["opacities"][:n], st["scales"][:n],
            st["rotations"][:n], torch.ones((n, 9), device="cuda"))
    with pytest.raises(RuntimeError, match="transMat_precomp.*viewmatrix"):
        pkg.rasterize_gaussians(*args, _settings(dict(st, viewmatrix=vm), W, H))
    out = pkg.rasterize_gaussians(*args, _settings(st, W, H))              # without the request the transform is taken as always
    assert out[0].shape == (2, H, W)
    # the C call: short, misaligned or missing scratch, a missing output; nothing is launched
    lib = _sf()._lib
    assert lib.lgsfpose_view_partial_floats(0) == 0 and lib.lgsfpose_view_partial_floats(-3) == 0
    assert lib.lgsfpose_view_partial_floats(1) == 16 and lib.lgsfpose_view_partial_floats(256) == 16 and lib.lgsfpose_view_partial_floats(257) == 32
    scene, W, H, radii, line, marks = _hook_case(260)
    b = ViewBackward(260, W, H, scene, radii)
    b.touched.write(marks)
    assert b.call(1) == 0
    untouched = b.out.read()
    assert b.call_view(partial_floats_arg=31) == -1                         # 260 surfels need 32 floats
    assert b.call_view(partials=C.c_void_p(b.partials.ptr.value + 4)) == -1  # not 16-byte aligned
    assert b.call_view(partials=None) == -1 and b.call_view(out=None) == -1
    assert b.call_view(gacc=None) < 0 and b.call_view(means=None) < 0 and b.call_view(view=None) < 0
    b.P = -1
    assert b.call_view() < 0
    assert same_bits(b.out.read(), untouched) and np.isnan(b.partials.read()).all()      # refused before any launch
    b.P = 0
    assert b.call_view(partials=None, partial_floats_arg=0) == 0
    assert not b.out.read().view(np.uint32).any()                           # sixteen zeros
    buf = Arr.filled(4096, np.uint32)
    p = buf.ptr
    out = Arr.filled(16, np.float32)

    def view(P=300, partials=p, n=64, out_=out.ptr, tm=None):
        return lib.lgsfpose_backward_view(P, 1, 0, 4, p, 64, 8, p, None, None, p, 1.0, p, tm, p, None, None, p, p, p, p, p, p, p, p, None, p, p, p, None,
                                          None, None, p, p, p, 0, _stream(), out_, partials, n)

    assert view(partials=None) == -1 and view(n=31) == -1 and view(P=-1) == -1 and view(out_=None) == -1 and view(tm=p) == -1
    assert view(partials=C.c_void_p(p.value + 8)) == -1
    _sync()
    assert np.isnan(out.read()).all()
    assert view(P=0, partials=None, n=0) == 0
    _sync()
    assert not out.read().view(np.uint32).any()
    buf.read()
