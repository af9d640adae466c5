"""Time the per-view evaluation of include/lidargs_metrics.h against the reference's metric block of training_report (train.py:314-371).

    python tools/time_view_metrics.py [--sizes 64x2650,128x4096] [--views 50] [--reps 20] [--warmup 3] [--out FILE.json]

Per size:
  native          view_metrics(), with and without the points meter part (include/lidargs_metrics.h)
  reference       the block as written, torch on the device: L1, PSNR, MAE, RMSE, two medians, structural_similarity on host copies
                  (scikit-image when it imports; otherwise tests/view_metrics_ref.ssim, the numpy restatement -- the row says which),
                  a fresh PointsMeter per view with its measure() (this project's device PointsMeter: one host read per view)
  loop            `--views` views: ViewMeter.update per view + one measure(), against the reference loop over the same views
Every time is the median of `--reps` runs after `--warmup`, each bracketed by torch.cuda.synchronize() (wall clock, includes the Python
wrappers and the scratch allocation); the loops run `--loop-reps` times.  --profile N: only N native calls (for rocprofv3 --kernel-trace)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "lidar-gs_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _gpu_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def _ssim_host():
    try:
        from skimage.metrics import structural_similarity
        return structural_similarity, "skimage"
    except Exception:
        import view_metrics_ref
        return (lambda a, b, data_range: view_metrics_ref.ssim(a, b)), "numpy restatement (scikit-image not importable)"


def make_view(H, W, seed, dev):
    import lidargs_scenes as sc
    rng = np.random.default_rng(seed)
    depth = (rng.gamma(2.0, 12.0, size=(1, H, W)) + 1.0).astype(np.float32)
    gt = np.stack([(rng.random((H, W)) > 0.15), rng.beta(2.0, 5.0, size=(H, W)),
                   depth[0] * (1.0 + 0.02 * rng.normal(size=(H, W)))]).astype(np.float32)
    render = np.stack([gt[1] + 0.1 * rng.normal(size=(H, W)), gt[0] * 0.8 + 0.3 * rng.random((H, W))]).astype(np.float32)
    beams = sc.beam_table(H, "waymo").astype(np.float32)
    return [torch.from_numpy(a).to(dev) for a in (render, depth, gt)] + [beams]


def reference_block(render, depth, gt, beams, ssim, dmin=5.0, dmax=80.0):
    """train.py:318-371 for one view, torch on the device; returns the 11 per-view values as the accumulators would add them."""
    import points_meter
    ray_drop = gt[0:1]
    gt_intensity = gt[1:2] * ray_drop
    mask = torch.where(render[1:2] > 0.5, 1, 0)
    image = torch.clamp(render[0:1], 0.0, 1.0) * mask
    l1 = torch.abs(image - gt_intensity).mean().double()
    mse = ((image - gt_intensity) ** 2).view(image.shape[0], -1).mean(1, keepdim=True)
    psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean().double()
    e = torch.abs(image - gt_intensity)
    in_mae, in_rmse, in_medae = e.mean(), torch.sqrt((e * e).mean()), e.median()
    in_ssim = ssim(image[0].detach().cpu().numpy(), gt_intensity[0].detach().cpu().numpy(), data_range=1.0)
    depth_render = torch.clamp(depth[0:1], dmin, dmax) * mask
    pm = points_meter.PointsMeter(scale=1, intrinsics=None, beam_inclinations=beams)
    pm.update(depth_render, gt[2:3] * ray_drop)
    cd_fs = pm.measure()
    d = torch.abs(depth_render - gt[2:3] * ray_drop)
    return [l1, psnr, in_ssim, in_mae, in_rmse, in_medae, cd_fs[0], cd_fs[1], d.mean(), d.median(), torch.sqrt((d * d).mean())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64x2650,128x4096")
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the rows as JSON here")
    a = ap.parse_args()
    import build_hip
    build_hip.build()
    import view_metrics as vm
    dev = torch.device("cuda")
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    if a.profile:
        for H, W in sizes:
            r, dp, g, b = make_view(H, W, 1, dev)
            bt = torch.from_numpy(b).to(dev)
            for _ in range(a.profile):
                vm.view_metrics(r, dp, g, beam_inclinations=bt)
            torch.cuda.synchronize()
        return
    ssim, ssim_kind = _ssim_host()
    res = dict(device=torch.cuda.get_device_name(0), build=build_hip.build_id(), reps=a.reps, warmup=a.warmup, ssim_host=ssim_kind, rows=[])
    for H, W in sizes:
        r, dp, g, b = make_view(H, W, 1, dev)
        bt = torch.from_numpy(b).to(dev)
        row = dict(H=H, W=W, ssim_host=ssim_kind)
        row["native_ms"] = _gpu_ms(lambda: vm.view_metrics(r, dp, g, beam_inclinations=bt), a.reps, a.warmup)
        row["native_no_points_ms"] = _gpu_ms(lambda: vm.view_metrics(r, dp, g, points_meter=False), a.reps, a.warmup)
        row["reference_ms"] = _gpu_ms(lambda: reference_block(r, dp, g, b, ssim), max(3, a.reps // 4), 1)
        views = [make_view(H, W, 100 + i, dev) for i in range(min(a.views, 10))]
        views = [views[i % len(views)] for i in range(a.views)]
        beams_dev = torch.from_numpy(views[0][3]).to(dev)

        def native_loop():
            meter = vm.ViewMeter(5.0, 80.0)
            for rv, dv, gv, _ in views:
                meter.update(rv, dv, gv, beams_dev)
            return meter.measure()

        def reference_loop():
            acc = [0.0] * 11
            for rv, dv, gv, bv in views:
                acc = [x + y for x, y in zip(acc, reference_block(rv, dv, gv, bv, ssim))]
            return [float(x) / len(views) for x in acc]

        row["views"] = a.views
        row["native_loop_ms"] = _gpu_ms(native_loop, a.loop_reps, 1)
        row["reference_loop_ms"] = _gpu_ms(reference_loop, a.loop_reps, 1)
        nl, rl = np.asarray(native_loop()), np.asarray(reference_loop())
        row["loop_max_rel_diff"] = float(np.nanmax(np.abs(nl - rl) / np.maximum(np.abs(rl), 1e-30)))
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
