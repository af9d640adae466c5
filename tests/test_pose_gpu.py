"""The gradient with respect to the sensor pose (dL/dviewmatrix): the pose form of the per-Gaussian chain (k_gaussian_backward_view), the
fold of its partial rows, `lgpose_backward_view` and the autograd plumbing of `GaussianRasterizer`, against tests/pose_ref.py (itself
held against float64 autograd of the whole forward by tests/test_pose_ref_cpu.py).

  (a) hook            `lgpose_debug_view_backward` on caller-supplied lines and marks against the float64 sum of the restatement's
                      per-Gaussian contributions, with its float32 run as the yardstick; on conic-only lines; on deterministic buffers
  (b) end to end      `viewmatrix.requires_grad_()` through GaussianRasterizer against the restatement fed the oracle's blend sums, and the
                      translation identity on HIP's own mean gradients
  (c) nothing moves   without the request the call is the one it was; with it every other gradient keeps its bits
  (d) modes           deterministic (twice, cloned buffers), median, enqueue-only frames, a captured graph
  (e) refusals

The bar of (a), per entry k of the matrix:  |got - sum_i c64[i,k]| <= 4 sum_i |c32[i,k] - c64[i,k]| + 10 * 2^-24 sum_i |c64[i,k]|.  The first term
is the project's factor 4 over an independent float32 evaluation of every contribution; the second covers the kernel's own summation in
float32 -- at most four adds per lane and six levels of the wave's tree, ten roundings of relative size 2^-24 on partial sums bounded by
sum |c| -- the fold of the partial rows being in double.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import lidargs_scenes as sc
import pose_ref
import preprocess_ref as ref
from test_deterministic_gpu import same_bits
from test_oracle_autograd_cpu import _close
from test_preprocess_gpu import ROWS, Arr, Backward, _binding, _chain_inputs, _chain_scene, _ptr, _stream, _sync
from util import GRAD_KEYS_SR, oracle_forward_backward, to_torch

pytestmark = pytest.mark.gpu

USED = [4 * r + k for r in range(4) for k in range(3)]
COLUMN3 = [3, 7, 11, 15]


def _lib():
    return _binding()._lib


def partial_floats(P):
    n = int(_lib().lgpose_view_partial_floats(P))
    assert n == 16 * ((P + 255) // 256)
    return n


class ViewBackward(Backward):
    """The arrays of a lgpose_debug_view_backward call: test_preprocess_gpu.Backward's, the sixteen outputs and the partial rows (NaN
    before the call), and -- `det` -- a mode word and the 64-bit lines of deterministic buffers."""

    def __init__(self, P, scene, mod=1.0, cov=None, det=False):
        super().__init__(P, 4, scene, mod, cov)
        self.out = Arr.filled(16, np.float32)
        self.partials = Arr.filled(partial_floats(P), np.float32)
        self.mode = Arr(np.array([1], np.uint32)) if det else None
        self.acc64 = Arr(np.zeros((P, 16), np.int64)) if det else None

    def call_view(self, partial_floats_arg=None, **null):
        i = self.ins
        a = dict(gacc=self.gacc.ptr, means=_ptr(i.get("means")), view=_ptr(i.get("view")), out=self.out.ptr, partials=self.partials.ptr)
        a.update(null)
        n = self.partials.shape[0] if partial_floats_arg is None else partial_floats_arg
        rc = _lib().lgpose_debug_view_backward(self.P, a["gacc"], a["means"], _ptr(i.get("scales")), self.mod, _ptr(i.get("rots")), _ptr(i.get("cov")),
                                                a["view"], *[_ptr(self.rows[k]) for k, _ in ROWS], self.tlist.ptr, self.tcount.ptr,
                                                _ptr(self.mode), _ptr(self.acc64), a["out"], a["partials"], n, _stream())
        _sync()
        return rc

    def run(self, line, marks):
        """lists and zeros (stage 1), the blend's fill, the pose form + fold -> (dL_dviewmatrix[16], partial rows, gradient rows)."""
        self.touched.write(marks)
        assert self.call(1) == 0, _binding()._err()
        self.gacc.write(line)
        assert self.call_view() == 0, _binding()._err()
        self.gacc.read(); self.tlist.read(); self.tcount.read()
        return self.out.read(), self.partials.read(), self.read_rows()


def _exact_view():
    """A rigid view whose arithmetic is exact in float32: a quarter turn about z and a mirror-free swap (entries 0, +-1), a dyadic
    translation.  The Gaussian at -t R^-1 then has range 0 exactly, whatever the order of the kernel's multiply-adds."""
    V = np.zeros((4, 4), np.float32)
    V[0, 1], V[1, 0], V[2, 2] = 1.0, -1.0, 1.0                            # pv = (-y, x, z) + t
    V[3, :3] = (0.5, -1.25, 0.25)
    V[3, 3] = 1.0
    return V


@functools.lru_cache(maxsize=None)
def _hook_case(P):
    """(scene, lines [P,16], marks): the Gaussians and per-slot magnitudes of test_preprocess_gpu._chain_inputs (one real backward's), N(0, 1)
    times those magnitudes in every line.  P > 1: the view is `_exact_view` with the Gaussians moved so that their view-space positions
    stay what they were, and Gaussian 5 sits at range 0.  Marks: region 0 whole (four trips of the 64-lane loop), region 1 empty where
    there are three regions or more, 40 % of the rest; the lines of unmarked Gaussians hold the same kind of numbers and must not be read."""
    base, base_line, _ = _chain_inputs()
    mag = np.sqrt((base_line.astype(np.float64) ** 2).mean(0))
    if P <= base_line.shape[0]:
        scene = {k: (v[:P].copy() if k in ("means3D", "scales", "rotations", "opacities", "colors") else v) for k, v in base.items()}
    else:
        scene, _, _ = _chain_scene(P)
    rng = np.random.default_rng([P, 77])
    line = (rng.normal(size=(P, 16)) * mag).astype(np.float32)
    marks = (rng.random(P) < 0.4).astype(np.uint8)
    marks[:256] = 1
    if P > 512:
        marks[256:512] = 0
    marks[P - 1] = 1
    if P > 1:
        V0 = np.asarray(scene["viewmatrix"], np.float64).reshape(4, 4)
        pv = scene["means3D"].astype(np.float64) @ V0[:3, :3] + V0[3, :3]
        V = _exact_view()
        scene["viewmatrix"] = V
        Vd = V.astype(np.float64)
        scene["means3D"] = ((pv - Vd[3, :3]) @ Vd[:3, :3].T).astype(np.float32)          # (orthonormal: the inverse is the transpose)
        scene["means3D"][5] = (-Vd[3, :3]) @ Vd[:3, :3].T
        marks[5] = 1
        p5 = scene["means3D"][5].astype(np.float64) @ Vd[:3, :3] + Vd[3, :3]
        assert not p5.any()
    return scene, line, marks


def _bar(c64, c32):
    return 4.0 * np.abs(c32 - c64).sum(0) + 10.0 * 2.0 ** -24 * np.abs(c64).sum(0)


def _check_against_float64(what, got, scene, line, marks, mod=1.0):
    import torch
    fed = line.astype(np.float64) * (marks != 0)[:, None]
    args = (fed, scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], mod)
    c64 = pose_ref.contributions(*args)
    c32 = pose_ref.contributions(*args, dtype=torch.float32)
    want, bar = c64.sum(0), _bar(c64, c32)
    err = np.abs(got.astype(np.float64) - want)
    for k in USED:
        print(f"[pose {what}] vm[{k:2d}] got {got[k]: .7e}  float64 {want[k]: .7e}  |diff| {err[k]:.2e}  bar {bar[k]:.2e} "
              f"(fp32 yardstick {bar[k] - 10.0 * 2.0 ** -24 * np.abs(c64[:, k]).sum():.2e})")
    assert np.isfinite(got).all(), what
    assert np.abs(want[USED]).min() > 0, what
    for k in USED:
        assert err[k] <= bar[k], (what, k, err[k], bar[k])
    assert not got[COLUMN3].view(np.uint32).any(), what                     # read by no kernel: +0


@pytest.mark.parametrize("P", [1, 260, 1025, 70001])
def test_hook_against_float64(P, hip_lib_built):
    """One lane; a short last region; one region past a four-wave block; more partial rows (274) than the fold has row groups."""
    scene, line, marks = _hook_case(P)
    b = ViewBackward(P, scene)
    got, partials, rows = b.run(line, marks)
    regions = (P + 255) // 256
    assert partials.size == 16 * regions and np.isfinite(partials).all()   # every region wrote its row over the NaNs
    part = partials.reshape(regions, 16)
    assert not part[:, COLUMN3].view(np.uint32).any()
    if P > 512:
        assert not part[1].view(np.uint32).any()                            # nothing touched: a row of +0
    _check_against_float64(f"P={P}", got, scene, line, marks)
    if P > 1:
        for k, a in rows.items():
            assert not a[5].view(np.uint32).any(), k                        # range 0: the rows stay as zeroed
    # the other outputs are the chain's, bit for bit
    plain = Backward(P, 4, scene)
    plain.touched.write(marks)
    assert plain.call(1) == 0
    plain.gacc.write(line)
    assert plain.call(2) == 0
    for k, a in plain.read_rows().items():
        assert same_bits(a, rows[k]), k
    # and a second call on the same arrays gives the same sixteen floats: no atomics on this path
    assert b.call_view() == 0
    assert same_bits(b.out.read(), got) and same_bits(b.partials.read(), partials)


def test_hook_on_conic_only_lines(hip_lib_built):
    """Slots 3-5 (dL/dconic) alone: the covariance path, through the damped conic, lies seven orders below the mean path and a missing
    gt_i (x) u_i term would hide inside the bar of the full lines.  Here it is the whole gradient of the rotation block."""
    P = 1025
    scene, line, marks = _hook_case(P)
    conic = np.zeros_like(line)
    conic[:, 3:6] = line[:, 3:6]
    got, partials, _ = ViewBackward(P, scene).run(conic, marks)
    assert np.isfinite(partials).all()
    _check_against_float64("conic only", got, scene, conic, marks)


def _det_lines(line, rng):
    """Deterministic buffers holding three terms per (Gaussian, slot): the float line = the largest |term| as bits, the 64-bit line = the
    sum of the terms on the grid that term fixes (csrc/lidargs_common.h det_encode) -> (tops as float32, acc64, the decoded float32 lines)."""
    w = np.array([0.5, 0.3, 0.2], np.float32)
    terms = (line[None] * w[:, None, None]).astype(np.float32) * np.where(rng.random((3,) + line.shape) < 0.3, -1.0, 1.0).astype(np.float32)
    top = np.abs(terms).max(0).astype(np.float32)
    e = np.maximum(top.view(np.uint32) >> 23, 1).astype(np.int64)
    q = np.rint(np.ldexp(terms.astype(np.float64), (165 - e)[None])).astype(np.int64)    # (exact products: |q| < 2^39)
    acc = q.sum(0)
    decoded = np.ldexp(acc.astype(np.float64), e - 165).astype(np.float32)
    return top, acc, decoded


def test_hook_on_deterministic_buffers(hip_lib_built):
    """Hand-built deterministic lines: the pose form reads them through det_decode, as the chain does.  The sixteen floats, the partial
    rows and every gradient row equal, bit for bit, what the plain float lines holding the decoded values give -- on the lists a stage-1
    call built from permuted marks."""
    P = 1025
    scene, line, marks = _hook_case(P)
    rng = np.random.default_rng(5)
    marks = marks.copy()
    marks[6:] = rng.permutation(marks[6:])                                  # (Gaussian 5 stays marked)
    top, acc, decoded = _det_lines(line, rng)
    assert np.isfinite(decoded).all() and not same_bits(decoded, top)
    want, want_part, want_rows = ViewBackward(P, scene).run(decoded, marks)
    b = ViewBackward(P, scene, det=True)
    b.acc64.write(acc)
    got, part, rows = b.run(top, marks)
    b.acc64.read(); b.mode.read()
    assert np.abs(got[USED]).min() > 0
    assert same_bits(got, want) and same_bits(part, want_part)
    for k, a in want_rows.items():
        assert same_bits(rows[k], a), k
    # the mode word decides, not the pointer: with the word cleared the float lines are read as they stand
    b.mode.write(np.array([0], np.uint32))
    assert b.call_view() == 0
    as_floats, _, _ = ViewBackward(P, scene).run(top, marks)
    assert same_bits(b.out.read(), as_floats)


# ---- (b) end to end -----------------------------------------------------------------------------------------------------------------
P_E2E, H_E2E, W_E2E = 2000, 16, 256


def _e2e_scene(kind):
    scene = sc.make_scene(kind, P_E2E, H_E2E, {"shell": 61, "street": 62}[kind], random_view=True)
    return scene, sc.upstream_grads(H_E2E, W_E2E, 61)


def _render(scene, grads, pose, only_pose=False, mod=1.0, retain=False):
    """One forward + backward through GaussianRasterizer; pose: the matrix requires grad.  -> dict of numpy results (+ the live tensors)."""
    import torch
    from diff_lidargs_rasterization import GaussianRasterizer
    st = to_torch(scene)
    P = st["means3D"].shape[0]
    leaves = {k: st[k].clone().requires_grad_(not only_pose) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    means2D = torch.zeros((P, 4), dtype=torch.float32, device="cuda", requires_grad=not only_pose)
    vm = st["viewmatrix"].clone().requires_grad_(pose)
    st = dict(st, viewmatrix=vm)
    rast = GaussianRasterizer(sc.raster_settings(st, W_E2E, H_E2E, 80, 0, mod))
    color, depth, occ, radii = rast(means3D=leaves["means3D"], means2D=means2D, shs=None, colors_precomp=leaves["colors"], opacities=leaves["opacities"],
                                    scales=leaves["scales"], rotations=leaves["rotations"], cov3D_precomp=None)
    g = [torch.from_numpy(x).cuda() for x in grads]
    torch.autograd.backward([color, depth, occ], g, retain_graph=retain)
    out = dict(color=color.detach().cpu().numpy(), depth=depth.detach().cpu().numpy(), occ=occ.detach().cpu().numpy(), radii=radii.cpu().numpy())
    if not only_pose:
        out.update(dL_dmeans3D=leaves["means3D"].grad.cpu().numpy(), dL_dmeans2D=means2D.grad.cpu().numpy(), dL_dcolors=leaves["colors"].grad.cpu().numpy(),
                   dL_dopacity=leaves["opacities"].grad.cpu().numpy(), dL_dscales=leaves["scales"].grad.cpu().numpy(),
                   dL_drotations=leaves["rotations"].grad.cpu().numpy())
    out["dL_dviewmatrix"] = None if vm.grad is None else vm.grad.cpu().numpy()
    out["live"] = (vm, [color, depth, occ], g)
    return out


def _translation_identity(what, scene, gvm, gw):
    """Row 3 of the gradient against HIP's own mean gradients rotated back: both sides are float32 evaluations of one sum of P terms,
    held to 1e-5 (about 170 ulp) of the terms' size sum_i sum_r |vm[4r+k]| |gw_i[r]|; a wrong term is O(1) of it."""
    V = np.asarray(scene["viewmatrix"], np.float64).reshape(4, 4)
    gw = gw.astype(np.float64)
    rhs = gw.sum(0) @ V[:3, :3]
    size = np.abs(gw).sum(0) @ np.abs(V[:3, :3])
    lhs = gvm.reshape(4, 4)[3, :3].astype(np.float64)
    print(f"[pose {what}] translation row {lhs}, mean gradients rotated back {rhs}, |diff| / size {np.abs(lhs - rhs) / size}")
    assert (np.abs(rhs) > 1e-3 * size).any()
    assert (np.abs(lhs - rhs) <= 1e-5 * size).all(), what


@pytest.mark.parametrize("kind", ["shell", "street"])
def test_end_to_end_against_the_restatement_on_the_oracles_sums(kind, hip_lib_built):
    scene, grads = _e2e_scene(kind)
    r = _render(scene, grads, pose=True)
    gvm = r["dL_dviewmatrix"]
    assert gvm is not None and gvm.shape == (4, 4) and gvm.dtype == np.float32
    o = oracle_forward_backward(scene, W_E2E, H_E2E, grads)
    f64 = ref.forward64(scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"])
    line = ref.line_from_oracle(o, np.nan_to_num(f64["u1"]), np.nan_to_num(f64["u2"]))
    want = pose_ref.contributions(line, scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"]).sum(0)
    got = gvm.reshape(16)
    print(f"[pose {kind}] got {got[USED]}\n[pose {kind}] want {want[USED]}")
    _close(f"dL_dviewmatrix {kind}", got[USED], want[USED])
    assert not got[COLUMN3].view(np.uint32).any()
    _translation_identity(kind, scene, gvm, r["dL_dmeans3D"])


def test_the_matrix_as_the_only_leaf(hip_lib_built):
    scene, grads = _e2e_scene("shell")
    r = _render(scene, grads, pose=True, only_pose=True)
    full = _render(scene, grads, pose=True)
    assert r["dL_dviewmatrix"] is not None
    _close("only leaf", r["dL_dviewmatrix"].reshape(16)[USED], full["dL_dviewmatrix"].reshape(16)[USED], rtol=1e-5, worst=1e-5)


# ---- (c) what must not move ---------------------------------------------------------------------------------------------------------
def test_nothing_moves_without_the_request_and_no_other_gradient_with_it(hip_lib_built, monkeypatch):
    """Under LIDARGS_DETERMINISTIC=1 (the default backward's float atomics do not repeat their own bits).  The binding's functions called
    directly -- the forward and `rasterize_gaussians_backward` with the arguments and the eight-element result they always had -- against
    the module with a matrix that does not require grad, and against the module with one that does."""
    import torch
    from diff_lidargs_rasterization import _C
    monkeypatch.setenv("LIDARGS_DETERMINISTIC", "1")
    scene, grads = _e2e_scene("street")
    calls = []
    real = _C.rasterize_gaussians_backward
    monkeypatch.setattr(_C, "rasterize_gaussians_backward", lambda *a, **kw: calls.append((kw, real(*a, **kw))) or calls[-1][1])
    off = _render(scene, grads, pose=False)
    assert off["dL_dviewmatrix"] is None
    assert list(calls[0][0]) == ["want_cov3D_grad"] and len(calls[0][1]) == 8      # the call it always was
    on = _render(scene, grads, pose=True)
    assert calls[1][0].get("want_viewmatrix_grad") is True and len(calls[1][1]) == 9
    monkeypatch.setattr(_C, "rasterize_gaussians_backward", real)
    st = to_torch(scene)
    e = torch.empty(0, device="cuda")
    fwd = _C.rasterize_gaussians(st["bg"], st["means3D"], st["colors"], st["opacities"], st["scales"], st["rotations"], 1.0, e, st["viewmatrix"],
                                 torch.eye(4, device="cuda"), H_E2E, W_E2E, st["beams"], e, 1, torch.zeros(3, device="cuda"), False, 80, 0, False)
    g = _C.rasterize_gaussians_backward(st["bg"], st["means3D"], fwd[4], st["colors"], st["scales"], st["rotations"], 1.0, e, st["viewmatrix"],
                                        torch.eye(4, device="cuda"), st["beams"], 1.0, 1.0, *[torch.from_numpy(x).cuda() for x in grads], e, 1,
                                        torch.zeros(3, device="cuda"), fwd[5], fwd[0], fwd[6], fwd[7], False, want_cov3D_grad=False)
    assert len(g) == 8
    direct = dict(color=fwd[1], depth=fwd[2], occ=fwd[3], radii=fwd[4], dL_dmeans2D=g[0], dL_dcolors=g[1], dL_dopacity=g[2], dL_dmeans3D=g[3],
                  dL_dscales=g[6], dL_drotations=g[7])
    assert np.abs(off["dL_dscales"]).max() > 0
    for k, t in direct.items():
        assert same_bits(off[k], t.cpu().numpy()), ("matrix without grad", k)
        assert same_bits(on[k], t.cpu().numpy()), ("matrix with grad", k)
    assert np.abs(on["dL_dviewmatrix"].reshape(16)[USED]).min() > 0


# ---- (d) modes ----------------------------------------------------------------------------------------------------------------------
def test_deterministic_twice_and_on_cloned_buffers(hip_lib_built, monkeypatch):
    import torch
    from diff_lidargs_rasterization import _C
    monkeypatch.setenv("LIDARGS_DETERMINISTIC", "1")
    scene, grads = _e2e_scene("street")
    r = _render(scene, grads, pose=True, retain=True)
    first = r["dL_dviewmatrix"]
    vm, outs, g = r["live"]
    vm.grad = None
    torch.autograd.backward(outs, g)                                        # retain_graph: the same forward's buffers once more
    assert same_bits(vm.grad.cpu().numpy(), first)
    again = _render(scene, grads, pose=True)["dL_dviewmatrix"]              # a second forward
    assert same_bits(again, first)
    st = to_torch(scene)
    e = torch.empty(0, device="cuda")
    fwd = _C.rasterize_gaussians(st["bg"], st["means3D"], st["colors"], st["opacities"], st["scales"], st["rotations"], 1.0, e, st["viewmatrix"],
                                 torch.eye(4, device="cuda"), H_E2E, W_E2E, st["beams"], e, 1, torch.zeros(3, device="cuda"), False, 80, 0, False)
    monkeypatch.delenv("LIDARGS_DETERMINISTIC")                             # the mode travels with the buffers
    radii, geom, binning, img = (t.clone() for t in (fwd[4], fwd[5], fwd[6], fwd[7]))
    out = _C.rasterize_gaussians_backward(st["bg"], st["means3D"], radii, st["colors"], st["scales"], st["rotations"], 1.0, e, st["viewmatrix"],
                                          torch.eye(4, device="cuda"), st["beams"], 1.0, 1.0, *g, e, 1, torch.zeros(3, device="cuda"), geom, fwd[0],
                                          binning, img, False, want_cov3D_grad=False, want_viewmatrix_grad=True)
    assert same_bits(out[8].cpu().numpy(), first)


def test_median_depth_buffers(hip_lib_built, monkeypatch):
    """LIDARGS_DEPTH=median: slot 9 of a line is what the median backward left there, and the pose form reads it as the chain does --
    the translation identity against HIP's own mean gradients holds under the same bar."""
    monkeypatch.setenv("LIDARGS_DEPTH", "median")
    scene, grads = _e2e_scene("shell")
    r = _render(scene, grads, pose=True)
    monkeypatch.delenv("LIDARGS_DEPTH")
    expected = _render(scene, grads, pose=True)
    assert not same_bits(r["depth"], expected["depth"])                     # the other depth
    assert np.isfinite(r["dL_dviewmatrix"]).all() and not r["dL_dviewmatrix"].reshape(16)[COLUMN3].view(np.uint32).any()
    _translation_identity("median", scene, r["dL_dviewmatrix"], r["dL_dmeans3D"])


def _enqueue_pose_setup():
    """test_parity_gpu._enqueue_setup with a matrix that requires grad -> (make, call, leaves, grads, viewmatrix leaf, scene)."""
    import torch
    from diff_lidargs_rasterization import GaussianRasterizer
    P, H, W, seed = 20000, 32, 600, 71
    scene = sc.make_scene("street", P, H, seed, random_view=True)
    st = to_torch(scene)
    vm = st["viewmatrix"].clone().requires_grad_(True)
    st = dict(st, viewmatrix=vm)
    leaves = {k: st[k].clone().requires_grad_(True) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    means2D = torch.zeros((P, 4), device="cuda", requires_grad=True)
    grads = [torch.from_numpy(g).cuda() for g in sc.upstream_grads(H, W, seed)]
    make = lambda: GaussianRasterizer(sc.raster_settings(st, W, H))
    call = lambda rast: rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], colors_precomp=leaves["colors"],
                             scales=leaves["scales"], rotations=leaves["rotations"])
    return make, call, list(leaves.values()) + [means2D], grads, vm, scene


def test_enqueue_only_frames(hip_lib_built):
    """The backward of an enqueue-only frame is lidargs_backward, so the request works there: the gradient of the ordinary frame within
    the summation-order band of the lines' float atomics (`_close`'s bars), and the translation identity on the frame's own mean gradients."""
    import torch
    make, call, leaves, grads, vm, scene = _enqueue_pose_setup()
    want = torch.autograd.grad(list(call(make())[:3]), [vm], grads)[0].cpu().numpy()
    eq = make()
    eq.enqueue_only = True
    call(eq)                                                                # learns the capacity (an ordinary frame)
    out = call(eq)
    assert eq._enqueue.frames == 1
    gvm, gw = torch.autograd.grad(list(out[:3]), [vm, leaves[0]], grads)
    assert not eq.enqueue_status()["overflow"]
    _close("enqueue-only", gvm.cpu().numpy().reshape(16)[USED], want.reshape(16)[USED])
    _translation_identity("enqueue-only", scene, gvm.cpu().numpy(), gw.cpu().numpy())


def test_inside_a_captured_graph(hip_lib_built):
    """Forward + backward with the request recorded in a HIP graph and replayed (no host read, no allocation in the library).  In a process
    of its own, for the reasons tests/test_parity_gpu.py::test_hip_graph_capture_of_forward_and_backward gives."""
    from util import run_child
    run_child(r"""
import gc
import numpy as np, torch
from test_pose_gpu import USED, _close, _enqueue_pose_setup, _translation_identity
make, call, leaves, grads, vm, scene = _enqueue_pose_setup()
inputs = leaves + [vm]
rast = make()
rast.enqueue_only = True
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):                         # warm-up off the default stream, as graph capture asks
    for _ in range(3):
        for t in inputs:
            t.grad = None
        out = call(rast)
        torch.autograd.backward(list(out[:3]), grads)
torch.cuda.current_stream().wait_stream(side)
torch.cuda.synchronize()
for t in inputs:
    t.grad = None
gc.collect()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    out = call(rast)
    torch.autograd.backward(list(out[:3]), grads)
replays = []
for _rep in range(2):
    graph.replay()
    torch.cuda.synchronize()
    replays.append((vm.grad.cpu().numpy().copy(), leaves[0].grad.cpu().numpy().copy()))
assert not rast.enqueue_status()["overflow"]
del graph
want = torch.autograd.grad(list(call(make())[:3]), [vm], grads)[0].cpu().numpy()
for gvm, gw in replays:
    assert gvm.shape == (4, 4) and np.isfinite(gvm).all()
    _close("graph replay", gvm.reshape(16)[USED], want.reshape(16)[USED])
    _translation_identity("graph replay", scene, gvm, gw)
print("OK")
""")


# ---- (e) refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib_built):
    lib = _lib()
    assert lib.lgpose_view_partial_floats(0) == 0 and lib.lgpose_view_partial_floats(-3) == 0
    assert lib.lgpose_view_partial_floats(1) == 16 and lib.lgpose_view_partial_floats(256) == 16 and lib.lgpose_view_partial_floats(257) == 32
    P = 300
    scene, line, marks = _hook_case(260)
    b = ViewBackward(260, scene)
    b.touched.write(marks)
    assert b.call(1) == 0
    untouched = b.out.read()
    assert b.call_view(partials=None) < 0                                   # NULL scratch
    assert b.call_view(partial_floats_arg=31) < 0                           # 260 Gaussians need 32 floats
    assert b.call_view(out=None) < 0 and b.call_view(gacc=None) < 0 and b.call_view(means=None) < 0 and b.call_view(view=None) < 0
    b.P = -1
    assert b.call_view() < 0
    assert same_bits(b.out.read(), untouched) and np.isnan(b.partials.read()).all()      # refused before any launch
    b.P = 0
    assert b.call_view(partials=None, partial_floats_arg=0) == 0
    assert not b.out.read().view(np.uint32).any()                           # sixteen zeros

    buf = Arr.filled(4096, np.uint32)
    p = buf.ptr
    out = Arr.filled(16, np.float32)

    def view(P=P, partials=p, n=64, out_=out.ptr):
        return lib.lgpose_backward_view(P, 1, 0, 4, p, 64, 8, p, None, p, p, 1.0, p, None, p, None, None, p, 1.0, 1.0, p, p, p, p, p, p, p,
                                         p, None, p, p, None, p, None, None, None, None, None, p, p, 0, _stream(), out_, partials, n)

    assert view(partials=None) < 0 and view(n=31) < 0 and view(P=-1) < 0 and view(out_=None) < 0
    _sync()
    assert np.isnan(out.read()).all()
    assert view(P=0, partials=None, n=0) == 0
    _sync()
    assert not out.read().view(np.uint32).any()
    buf.read()
