"""The per-view evaluation on the device (lidar-gs_amd/view_metrics.py -> lidargs_view_metrics) against the numpy restatement
(tests/view_metrics_ref.py), the reference's torch expressions of train.py:318-363 run on the same device tensors, and the fixture
made by executing the reference's loop (tests/golden/make_view_metrics_golden.py).

Held: the medians bit for bit against torch.median; slots 6 and 7 bit for bit against points_metrics() on torch's depth_r / gt_depth;
means (float64 sums rounded to float32, against torch's float32 reductions) to 2e-6 relative; PSNR to 1e-4 dB; SSIM to 2e-6 absolute
(float64 window sums in another order than the restatement's cumulative sums: a window mean may round to the other float32 neighbour).
NaN wherever the reference gives NaN."""
import os

import numpy as np
import pytest

import view_metrics_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "view_metrics_golden.npz"))


def _close(got, want, slot, rel=2e-6):
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    if np.isinf(want) or np.isinf(got):
        return got == want
    if slot in (5, 9):
        return got == want
    if slot == 1:
        return abs(got - want) <= 1e-4
    if slot == 2:
        return abs(got - want) <= 2e-6
    return abs(got - want) <= rel * abs(want)


def torch_block(render, depth, gt, dmin, dmax):
    """train.py:318-363 as the reference writes it, on the device tensors (PSNR as utils/image_utils.py, L1 as utils/loss_utils.py)."""
    import torch
    ray_drop = gt[0:1]
    gt_intensity = gt[1:2] * ray_drop
    render_raydrop_mask = torch.where(render[1:2] > 0.5, 1, 0)
    image = torch.clamp(render[0:1], 0.0, 1.0) * render_raydrop_mask
    l1 = torch.abs(image - gt_intensity).mean()
    mse = ((image - gt_intensity) ** 2).view(image.shape[0], -1).mean(1, keepdim=True)
    psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    e = torch.abs(image - gt_intensity)
    depth_render = torch.clamp(depth[0:1], dmin, dmax) * render_raydrop_mask
    gt_depth = gt[2:3] * ray_drop
    d = torch.abs(depth_render - gt_depth)
    vals = [l1, psnr, None, e.mean(), torch.sqrt((e * e).mean()), e.median(), None, None, d.mean(), d.median(), torch.sqrt((d * d).mean())]
    return [None if v is None else float(v) for v in vals], depth_render[0], gt_depth[0]


def check(render, depth, gt, beams, dmin=5.0, dmax=80.0):
    """Native against torch on the device and the restatement; returns the native row."""
    import torch
    import points_meter
    import view_metrics
    r, dp, g = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (render, depth, gt))
    bt = torch.from_numpy(np.ascontiguousarray(beams, np.float32)).cuda()
    got = view_metrics.view_metrics(r, dp, g, beam_inclinations=bt, depth_min=dmin, depth_max=dmax)
    assert got.dtype == torch.float64 and got.shape == (11,) and got.is_cuda
    got = got.cpu().numpy()
    tv, depth_r, gt_depth = torch_block(r, dp, g, dmin, dmax)
    pm = points_meter.points_metrics(depth_r, gt_depth, beam_inclinations=bt).cpu().numpy()
    ref = R.view_metrics(render, depth, gt, dmin, dmax, points=lambda a, b: (float(pm[0]), float(pm[1])))
    bad = []
    for k in range(11):
        if not _close(got[k], ref[k], k):
            bad.append(("restatement", R.NAMES[k], got[k], ref[k]))
        if tv[k] is not None and not _close(got[k], tv[k], k):
            bad.append(("torch", R.NAMES[k], got[k], tv[k]))
    for k in (6, 7):                                           # bit for bit with the points meter on torch's prepared images
        same = (np.isnan(got[k]) and np.isnan(pm[k - 6])) or (got[k] == float(pm[k - 6]) and float(np.float32(got[k])) == got[k])
        if not same:
            bad.append(("points_metrics", R.NAMES[k], got[k], pm[k - 6]))
    assert not bad, bad
    return got


def synthetic(H, W, seed, zeros=0.0):
    import lidargs_scenes as sc
    rng = np.random.default_rng(seed)
    depth = (rng.gamma(2.0, 12.0, size=(1, H, W)) + 1.0).astype(np.float32)
    gt = np.stack([(rng.random((H, W)) > 0.15), rng.beta(2.0, 5.0, size=(H, W)),
                   depth[0] * (1.0 + 0.02 * rng.normal(size=(H, W)))]).astype(np.float32)
    render = np.stack([gt[1] + 0.1 * rng.normal(size=(H, W)), gt[0] * 0.8 + 0.3 * rng.random((H, W))]).astype(np.float32)
    if zeros:
        z = rng.random((H, W)) < zeros
        render[0][z] = 0.0; gt[1][z] = 0.0; render[1][z] = 0.9; gt[0][z] = 1.0; depth[0][z] = 5.0; gt[2][z] = 5.0
    return render, depth, gt, sc.beam_table(H, "waymo").astype(np.float32)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e"])
def test_matches_the_reference_fixture(tag, hip_lib_built):
    import torch
    import view_metrics
    render, depth, gt, beams = (GOLD[f"{tag}_{k}"] for k in ("render", "depth", "gt", "beams"))
    dmin, dmax = (float(v) for v in GOLD[f"{tag}_depth_range"])
    got = view_metrics.view_metrics(*(torch.from_numpy(a).cuda() for a in (render, depth, gt)), beam_inclinations=beams,
                                    depth_min=dmin, depth_max=dmax).cpu().numpy()
    want = GOLD[f"{tag}_out"]
    bad = [(R.NAMES[k], got[k], want[k]) for k in range(11) if k not in (6, 7) and not _close(got[k], want[k], k)]
    assert abs(got[6] - want[6]) <= 2e-5 * abs(want[6]) and abs(got[7] - want[7]) <= 0.05     # the points meter's own tolerances (test_points_meter.py)
    assert not bad, bad
    check(render, depth, gt, beams, dmin, dmax)


@pytest.mark.parametrize("H,W", [(7, 7), (7, 9), (8, 8), (33, 1001), (10, 1000), (64, 2650)])
def test_odd_and_even_sizes(H, W, hip_lib_built):
    check(*synthetic(H, W, H * 7919 + W))


@pytest.mark.parametrize("H,W,P", [(64, 2650, 150_000), (128, 4096, 300_000)])
def test_street_frames_from_the_rasterizer(H, W, P, hip_lib_built):
    """A rendered frame as render_pkg: intensity / ray-drop from the rasterizer's colour channels, its depth; the ground truth a second
    render of a perturbed scene."""
    import lidargs_scenes as sc
    from util import hip_forward_backward
    beams = sc.beam_table(H, "waymo").astype(np.float32)
    scene = sc.make_scene("street", P, H, 3, beams=beams)
    a = hip_forward_backward(scene, W, H)
    rng = np.random.default_rng(4)
    other = dict(scene)
    other["means3D"] = (scene["means3D"] + 0.05 * rng.normal(size=scene["means3D"].shape)).astype(np.float32)
    b = hip_forward_backward(other, W, H)
    render = np.stack([a["color"][0], a["color"][1] + 0.4 * a["occ"][0]]).astype(np.float32)
    depth = a["depth"][:1].astype(np.float32)
    gt = np.stack([(b["occ"][0] > 0.5), b["color"][0], b["depth"][0]]).astype(np.float32)
    got = check(render, depth, gt, beams)
    assert np.isfinite(got).all()


def test_every_ray_dropped(hip_lib_built):
    """Render and ground truth drop every ray: no error at all -> PSNR +inf, SSIM 1, medians 0; both clouds empty -> the points meter's
    NaN chamfer distance and F-score 0."""
    render, depth, gt, beams = synthetic(16, 64, 5)
    render[1] = 0.0; gt[0] = 0.0
    got = check(render, depth, gt, beams)
    assert got[1] == np.inf and got[2] == 1.0 and got[5] == 0.0 and got[9] == 0.0 and got[0] == 0.0 and got[8] == 0.0
    assert np.isnan(got[6]) and got[7] == 0.0


def test_range_edges_and_nan(hip_lib_built):
    """Intensities outside [0, 1], ray-drop exactly 0.5 (dropped: strict >), NaN in render[0] (through the clamp and the mask), NaN in
    render[1] (not > 0.5: dropped), NaN in the depth (through its clamp)."""
    render, depth, gt, beams = synthetic(24, 300, 6)
    render[0][:, :40] = 1.7; render[0][:, 40:80] = -0.3
    render[1][::3, ::5] = 0.5
    got = check(render, depth, gt, beams)
    assert np.isfinite(got).all()
    r2 = render.copy(); r2[1][4, 7] = np.nan                       # a dropped ray only
    assert np.isfinite(check(r2, depth, gt, beams)[[0, 1, 2, 5]]).all()
    r3 = render.copy(); r3[0][5, 9] = np.nan
    got = check(r3, depth, gt, beams)
    assert np.isnan(got[[0, 1, 2, 3, 4, 5]]).all() and np.isfinite(got[[8, 9, 10]]).all()
    d2 = depth.copy(); d2[0][7, 11] = np.nan
    r4 = render.copy(); r4[1][7, 11] = 0.9
    got = check(r4, d2, gt, beams)
    assert np.isnan(got[[8, 9, 10]]).all() and np.isfinite(got[[0, 1, 2, 5]]).all()


def test_many_ties(hip_lib_built):
    got = check(*synthetic(32, 700, 7, zeros=0.7))
    assert got[5] == 0.0 and got[9] == 0.0
    got = check(*synthetic(32, 701, 8, zeros=0.3))                  # the median sits above the tie block
    assert got[5] > 0.0


def test_reproducible_and_graph_capturable(hip_lib_built):
    import torch
    import view_metrics
    render, depth, gt, beams = synthetic(64, 2650, 9)
    r, dp, g = (torch.from_numpy(a).cuda() for a in (render, depth, gt))
    bt = torch.from_numpy(beams).cuda()
    a = view_metrics.view_metrics(r, dp, g, beam_inclinations=bt).cpu().numpy()
    b = view_metrics.view_metrics(r, dp, g, beam_inclinations=bt).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    out = torch.full((11,), -1.0, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        view_metrics.view_metrics(r, dp, g, beam_inclinations=bt, out=out)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    out.fill_(-1.0)
    with torch.cuda.graph(graph):
        view_metrics.view_metrics(r, dp, g, beam_inclinations=bt, out=out)
    out.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == a.tobytes()
    r.copy_(torch.from_numpy(synthetic(64, 2650, 10)[0]).cuda())             # new inputs in place: the replay follows them
    graph.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == view_metrics.view_metrics(r, dp, g, beam_inclinations=bt).cpu().numpy().tobytes()


def test_view_meter_is_the_mean_of_the_rows(hip_lib_built):
    import torch
    import view_metrics
    meter = view_metrics.ViewMeter(5.0, 80.0)
    rows = []
    for seed in range(4):
        render, depth, gt, beams = synthetic(16, 256, 20 + seed)
        args = [torch.from_numpy(a).cuda() for a in (render, depth, gt)]
        meter.update(*args, beams)
        rows.append(view_metrics.view_metrics(*args, beam_inclinations=beams).cpu().numpy())
    got = meter.measure()
    assert got.dtype == np.float64 and got.shape == (11,)
    np.testing.assert_allclose(got, np.mean(rows, 0), rtol=1e-15, atol=0)
    meter.clear()
    assert np.isnan(meter.measure()).all()


def test_without_the_points_meter(hip_lib_built):
    import torch
    import view_metrics
    render, depth, gt, beams = synthetic(16, 256, 30)
    args = [torch.from_numpy(a).cuda() for a in (render, depth, gt)]
    full = view_metrics.view_metrics(*args, beam_inclinations=beams).cpu().numpy()
    part = view_metrics.view_metrics(*args, points_meter=False).cpu().numpy()
    assert np.isnan(part[[6, 7]]).all()
    keep = [0, 1, 2, 3, 4, 5, 8, 9, 10]
    assert part[keep].tobytes() == full[keep].tobytes()
