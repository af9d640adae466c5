"""GPU tests of the sweep-motion compensation (lidar-gs_amd/sweep_motion.py -> lgsweep_forward / lgsweep_backward of liblidargs_hip.so,
csrc/sweep_motion.hip) against tests/sweep_ref.py, the float64 restatement of include_sweep/lidargs_sweep.h (itself held against the matrix
exponential, a sweep assembled column by column and gradcheck by tests/test_sweep_ref_cpu.py).

The bar, per compared array (x', dL_dmeans3D, dL_dtwist, dL_dviewmatrix for random upstream gradients), as in tests/test_tcnn_gpu.py:
    max|native - ref64| <= max(4 max|float32 chain - ref64|, 16 * 2^-24 max|ref64|)
where the float32 chain is the restatement run on the same float32 inputs as framework ops.  The worst ratio err / bound over the suite
is printed per case and quoted in DESIGN.md 4f."""
import numpy as np
import pytest
import torch

import lidargs_scenes as sc
import sweep_ref as R
from test_deterministic_gpu import same_bits
from util import run_child, surfel_scene, to_torch

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 4099, 70001]             # region edges of the partial rows (256), several fold rows (more than 32 regions), one lane
ITERATIONS = [1, 3, 4]
SWEEPS = [(-0.5, 0.5), (0.5, -0.5), (0.0, 1.0)]
FLOOR = 16 * 2.0 ** -24
COLUMN3 = [3, 7, 11, 15]


def sweep_motion():
    import sweep_motion as m
    return m


def _vm(seed=18):
    return torch.from_numpy(sc.rigid_viewmatrix(np.random.default_rng(seed)))          # what make_scene(random_view=True) draws


def _case(P, seed, seam=False, twist=R.TWIST):
    """float32 (x, vm, xi, g) on the host: sensor-frame points of the restatement's generator carried to the world of a random view."""
    vm = _vm()
    x = R.world_points(R.points(P, seed, margin=1.1e-3, seam=seam), vm.double()).float()
    g = torch.randn(P, 3, generator=torch.Generator().manual_seed(seed + 1))
    return x, vm, torch.tensor(twist, dtype=torch.float32), g


def native(x, vm, xi, g, sweep, n, want=(True, True, True)):
    """(x', dL_dmeans3D, dL_dviewmatrix, dL_dtwist) of the product on the device, as host tensors (None where not asked for)."""
    leaves = [t.cuda().requires_grad_(w) for t, w in zip((x, vm, xi), want)]
    out = sweep_motion().compensate(*leaves, sweep=sweep, iterations=n)
    if any(want):
        out.backward(g.cuda())
    return [out.detach().cpu()] + [None if t.grad is None else t.grad.cpu() for t in leaves]


def judge(what, got, x, vm, xi, g, sweep, n, margin=1e-3):
    """The bar of the module docstring on every array of `got` that is not None; -> the worst err / bound."""
    R.compensate(x.double(), vm.double(), xi.double(), sweep, n, margin=margin)        # asserts the domain: no case is left out
    f64 = R.vjp(x.double(), vm.double(), xi.double(), g.double(), sweep, n)
    f32 = R.vjp(x, vm, xi, g, sweep, n)
    worst = 0.0
    for name, a, b, r in zip(("x'", "dL_dmeans3D", "dL_dviewmatrix", "dL_dtwist"), got, f32, f64):
        if a is None:
            continue
        assert a.dtype == torch.float32 and a.shape == r.shape, name
        e_n, e_f = float((a.double() - r).abs().max()), float((b.double() - r).abs().max())
        bound = max(4 * e_f, FLOOR * float(r.abs().max()))
        print(f"{what} {name}: native {e_n:.3e}, framework float32 {e_f:.3e}, bound {bound:.3e}, err / bound {e_n / bound:.3f}")
        assert e_n <= bound, (what, name, e_n, e_f, bound)
        worst = max(worst, e_n / bound)
    if got[2] is not None:
        assert not got[2].reshape(16)[COLUMN3].numpy().view(np.uint32).any()             # column 3: +0
    return worst


@pytest.mark.parametrize("sweep", SWEEPS)
@pytest.mark.parametrize("n", ITERATIONS)
@pytest.mark.parametrize("P", SIZES)
def test_against_float64_and_the_framework_yardstick(P, n, sweep, hip_lib_built):
    x, vm, xi, g = _case(P, 100 + P % 97)
    judge(f"P={P} n={n} sweep={sweep}", native(x, vm, xi, g, sweep, n), x, vm, xi, g, sweep, n)


@pytest.mark.parametrize("sweep", SWEEPS)
@pytest.mark.parametrize("n", ITERATIONS)
def test_seam_scene(n, sweep, hip_lib_built):
    # (columns that run against time: the twist reversed as well, so that the points cross the seam as they do for the other sweeps)
    x, vm, xi, g = _case(512, 9, seam=True, twist=R.TWIST if sweep[0] < sweep[1] else tuple(-k for k in R.TWIST))
    s = R.iterate(x.double() @ vm.double()[:3, :3] + vm.double()[3, :3], xi.double(), sweep, n)
    if n > 1:
        assert int(((s < 0) | (s >= 1)).sum()) >= 20                                     # the seam rule is at work
    judge(f"seam n={n} sweep={sweep}", native(x, vm, xi, g, sweep, n), x, vm, xi, g, sweep, n, margin=0.9e-3)


def test_a_large_rotation_takes_the_closed_form_branch(hip_lib_built):
    """|w| |t| up to 1.3 rad: theta^2 > 1, where the kernels leave the series for sincos."""
    x, vm, xi, g = _case(4099, 33, twist=(0.9, -1.4, 2.0, 1.5, 0.2, 0.05))
    judge("large rotation", native(x, vm, xi, g, (-0.5, 0.5), 2), x, vm, xi, g, (-0.5, 0.5), 2)


def test_reduced_gradients_repeat_their_bits(hip_lib_built):
    x, vm, xi, g = _case(70001, 5)
    other = _case(4099, 6)
    first = native(x, vm, xi, g, (-0.5, 0.5), 3)
    for k in range(3):
        if k == 2:
            native(*other, (0.0, 1.0), 4)                                               # an unrelated call in between
            torch.randn(1 << 20, device="cuda").sum().item()
        again = native(x, vm, xi, g, (-0.5, 0.5), 3)
        for a, b in zip(first, again):
            assert same_bits(a.numpy(), b.numpy())


def test_zero_twist_is_the_identity(hip_lib_built):
    x, vm, _, g = _case(4099, 7)
    xi = torch.zeros(6)
    got = native(x, vm, xi, g, (-0.5, 0.5), 3)
    ulp = 2.0 ** -23 * float(x.abs().max())
    assert float((got[0] - x).abs().max()) <= 2 * ulp
    # dL_dviewmatrix is x^T g_y - x'^T g_y: two sums of this size that cancel
    size = float((x.double().abs().T @ g.double().abs()).max())
    print("zero twist: dL_dviewmatrix", got[2].abs().max().item(), "against the floor", FLOOR * size)
    assert float(got[2].abs().max()) <= FLOOR * size
    assert float((got[1] - g).abs().max()) <= FLOOR * float(g.abs().max())
    judge("zero twist", [got[0], got[1], None, got[3]], x, vm, xi, g, (-0.5, 0.5), 3)     # dL_dtwist is not zero there


@pytest.mark.parametrize("want", [(True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)])
def test_only_the_requested_gradients(want, hip_lib_built):
    x, vm, xi, g = _case(4099, 8)
    full = native(x, vm, xi, g, (-0.5, 0.5), 3)
    got = native(x, vm, xi, g, (-0.5, 0.5), 3, want=want)
    assert same_bits(got[0].numpy(), full[0].numpy())
    for w, a, b in zip(want, got[1:], full[1:]):
        assert (a is not None) == w
        if w:
            assert same_bits(a.numpy(), b.numpy())


def test_no_grad_saves_nothing_and_strided_inputs_are_made_contiguous(hip_lib_built):
    m = sweep_motion()
    x, vm, xi, g = (t.cuda() for t in _case(4099, 10))
    want = m.compensate(x, vm, xi)
    assert want.grad_fn is None
    with torch.no_grad():
        out = m.compensate(x.clone().requires_grad_(True), vm, xi)
    assert out.grad_fn is None and not out.requires_grad and same_bits(out.cpu().numpy(), want.cpu().numpy())
    xs = x.t().contiguous().t()                                                          # [P, 3] with strides (1, P)
    vms = vm.t().contiguous().t()
    xis = torch.stack([xi, xi], 1)[:, 0]
    assert not xs.is_contiguous() and not vms.is_contiguous() and not xis.is_contiguous()
    leaves = [t.detach().requires_grad_(True) for t in (xs, vms, xis)]
    assert not any(t.is_contiguous() for t in leaves)
    out = m.compensate(*leaves)
    out.backward(g)
    ref = native(x.cpu(), vm.cpu(), xi.cpu(), g.cpu(), (-0.5, 0.5), 3)
    assert same_bits(out.detach().cpu().numpy(), ref[0].numpy())
    for t, r in zip(leaves, ref[1:]):
        assert t.grad.shape == r.shape and same_bits(t.grad.cpu().numpy(), r.numpy())


def test_python_refusals(hip_lib_built, monkeypatch):
    m = sweep_motion()
    x, vm, xi, _ = (t.cuda() for t in _case(16, 11))
    for bad in ((x.cpu(), vm, xi), (x, vm.cpu(), xi), (x, vm, xi.cpu())):
        with pytest.raises(RuntimeError, match="HIP device"):
            m.compensate(*bad)
    for bad in ((x.double(), vm, xi), (x, vm.double(), xi), (x, vm, xi.half())):
        with pytest.raises(RuntimeError, match="Float"):
            m.compensate(*bad)
    for bad in ((x[:, :2], vm, xi), (x.reshape(-1), vm, xi), (x, vm[:3], xi), (x, vm, xi[:5]), (x, vm, xi.reshape(2, 3))):
        with pytest.raises(RuntimeError, match="dimensions"):
            m.compensate(*bad)
    for n in (0, 5, -1, 2.0, True):
        with pytest.raises(ValueError, match="iterations"):
            m.compensate(x, vm, xi, iterations=n)
    with pytest.raises(ValueError, match="finite"):
        m.compensate(x, vm, xi, sweep=(0.0, float("inf")))
    monkeypatch.setattr(m, "_Compensate", None)                                          # P == 0: no native call
    out = m.compensate(x[:0], vm, xi)
    assert out.shape == (0, 3) and out.dtype == torch.float32 and out.is_cuda


def test_an_empty_call_writes_the_reduced_gradients_as_zeros(hip_lib_built):
    """P = 0 at the C boundary (the Python side never gets there): returns 0, the reduced gradients that were asked for are zeros."""
    import lidargs_abi
    m = sweep_motion()
    _, vm, xi, _ = (t.cuda() for t in _case(1, 13))
    out = torch.full((32,), float("nan"), device="cuda")
    args = lambda g_xi, g_vm: (0, None, lidargs_abi.ptr(vm), lidargs_abi.ptr(xi), -0.5, 0.5, 3, None, None, g_xi, g_vm, None, 0, lidargs_abi.stream(vm))
    assert m._lib.lgsweep_forward(0, None, lidargs_abi.ptr(vm), lidargs_abi.ptr(xi), -0.5, 0.5, 3, None, lidargs_abi.stream(vm)) == 0
    assert m._lib.lgsweep_backward(*args(lidargs_abi.ptr(out[16:22]), None)) == 0
    torch.cuda.synchronize()
    assert not out[16:22].cpu().numpy().view(np.uint32).any() and bool(torch.isnan(out[:16]).all()) and bool(torch.isnan(out[22:]).all())
    assert m._lib.lgsweep_backward(*args(None, lidargs_abi.ptr(out[:16]))) == 0
    torch.cuda.synchronize()
    assert not out[:22].cpu().numpy().view(np.uint32).any() and bool(torch.isnan(out[22:]).all())


def test_inside_a_captured_graph(hip_lib_built):
    """Forward + backward recorded in one HIP graph and replayed: no host read, no allocation in the library; the replays give the eager
    bits.  In a process of its own, for the reasons tests/test_parity_gpu.py::test_hip_graph_capture_of_forward_and_backward gives."""
    run_child(r"""
import torch
import sweep_motion
from test_deterministic_gpu import same_bits
from test_sweep_gpu import _case
x, vm, xi, g = (t.cuda() for t in _case(70001, 12))
leaves = [t.requires_grad_(True) for t in (x, vm, xi)]
def step():
    out = sweep_motion.compensate(*leaves, sweep=(0.5, -0.5), iterations=3)
    out.backward(g)
    return out
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):                         # warm-up off the default stream, as graph capture asks
    for _ in range(3):
        for t in leaves:
            t.grad = None
        step()
torch.cuda.current_stream().wait_stream(side)
torch.cuda.synchronize()
for t in leaves:
    t.grad = None
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    out = step()
replays = []
for _rep in range(2):
    graph.replay()
    torch.cuda.synchronize()
    replays.append([out.detach().cpu().numpy().copy()] + [t.grad.cpu().numpy().copy() for t in leaves])
del graph
for t in leaves:
    t.grad = None
eager = step()
want = [eager.detach().cpu().numpy()] + [t.grad.cpu().numpy() for t in leaves]
for rep in replays:
    for a, b in zip(rep, want):
        assert a.shape == b.shape and same_bits(a, b)
print("OK")
""")


# ---- end to end: compensate -> a rasterizer -> a loss -> backward() -------------------------------------------------------------------------
P_E2E, H_E2E, W_E2E = 4096, 32, 512
SEED_E2E, MARGIN_E2E = 46, 2e-4        # a street scene whose Gaussians keep 2 m from the sensor's axis and 2.6e-4 rad from the seam (asserted by judge)


def _loss(outs):
    return sum((o * torch.linspace(0.5, 1.5, o.numel(), device=o.device).view_as(o)).sum() for o in outs)


def _e2e(monkeypatch, surfel):
    """-> (x, vm, xi) float32 on the host, the gradient g the rasterizer handed back at x', twist.grad, viewmatrix.grad, and the
    rasterizer's own pose gradient on the same warped means (a second run, x' as a leaf; the 3-D rasterizer only: under
    LIDARGS_DETERMINISTIC=1, which the surfel entry points refuse, the second run repeats the bits of the first -- the default backward's
    float atomics do not)."""
    if not surfel:
        monkeypatch.setenv("LIDARGS_DETERMINISTIC", "1")
    m = sweep_motion()
    if surfel:
        from diff_lidargs_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
        scene = surfel_scene("street", P_E2E, H_E2E, SEED_E2E)
    else:
        from diff_lidargs_rasterization import GaussianRasterizer
        scene = sc.make_scene("street", P_E2E, H_E2E, SEED_E2E, random_view=True)
    st = to_torch(scene)
    xi = torch.tensor(R.TWIST, device="cuda").requires_grad_(True)

    def render(means3D, vm):
        means2D = torch.zeros((P_E2E, 4), device="cuda", requires_grad=True)
        if surfel:
            rast = GaussianRasterizer(GaussianRasterizationSettings(
                image_height=H_E2E, image_width=W_E2E, bg=st["bg"], scale_modifier=1.0, depth_threshold=0.0, viewmatrix=vm,
                projmatrix=torch.eye(4, device="cuda"), sh_degree=1, campos=torch.zeros(3, device="cuda"), prefiltered=False,
                beam_inclinations=st["beams"], lidar_far=80, lidar_near=0, debug=False))
            color, _radii, others, _pixels = rast(means3D=means3D, means2D=means2D, opacities=st["opacities"], shs=None, colors_precomp=st["colors"],
                                                  scales=st["scales"], rotations=st["rotations"])
            return _loss([color, others])
        rast = GaussianRasterizer(sc.raster_settings(dict(st, viewmatrix=vm), W_E2E, H_E2E))
        color, depth, occ, _radii = rast(means3D=means3D, means2D=means2D, shs=None, colors_precomp=st["colors"], opacities=st["opacities"],
                                         scales=st["scales"], rotations=st["rotations"], cov3D_precomp=None)
        return _loss([color, depth, occ])

    x = st["means3D"].clone().requires_grad_(True)
    vm = st["viewmatrix"].clone().requires_grad_(True)
    warped = m.compensate(x, vm, xi)
    seen = []
    warped.register_hook(lambda grad: seen.append(grad.detach().clone()))
    render(warped, vm).backward()
    assert len(seen) == 1
    raster_share = None
    if not surfel:
        leaf = warped.detach().clone().requires_grad_(True)
        vm2 = st["viewmatrix"].clone().requires_grad_(True)
        render(leaf, vm2).backward()
        assert same_bits(seen[0].cpu().numpy(), leaf.grad.cpu().numpy())
        raster_share = vm2.grad.cpu()
    return [t.detach().cpu() for t in (x, vm, xi)], seen[0].cpu(), xi.grad.cpu(), vm.grad.cpu(), raster_share, x.grad.cpu()


def test_end_to_end_through_the_rasterizer(hip_lib_built, monkeypatch):
    (x, vm, xi), g, g_xi, g_vm, g_vm_raster, g_x = _e2e(monkeypatch, surfel=False)
    assert float(g.abs().max()) > 0 and torch.isfinite(g_vm).all()
    # the chain identity: twist.grad, means3D.grad and the warp's share of viewmatrix.grad are the restatement's VJP fed the rasterizer's gradient at x'
    judge("end to end", [None, g_x, None, g_xi], x, vm, xi, g, (-0.5, 0.5), 3, margin=MARGIN_E2E)
    share = native(x, vm, xi, g, (-0.5, 0.5), 3)[2]
    judge("end to end, the warp's share", [None, None, share, None], x, vm, xi, g, (-0.5, 0.5), 3, margin=MARGIN_E2E)
    assert same_bits(g_vm.numpy(), (g_vm_raster + share).numpy())                        # ... which simply adds to the rasterizer's pose gradient
    assert float(g_vm_raster.abs().max()) > 0 and float(share.abs().max()) > 0


def test_end_to_end_through_the_surfel_rasterizer(hip_lib_built, monkeypatch):
    (x, vm, xi), g, g_xi, g_vm, g_vm_raster, g_x = _e2e(monkeypatch, surfel=True)
    assert all(bool(torch.isfinite(t).all()) for t in (g, g_xi, g_vm, g_x)) and float(g.abs().max()) > 0
    judge("surfel end to end", [None, g_x, None, g_xi], x, vm, xi, g, (-0.5, 0.5), 3, margin=MARGIN_E2E)
