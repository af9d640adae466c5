"""Device time of the range-view conversion (lidar-gs_amd/range_view.py) at 64 x 2650, beside the same result as framework ops on the same
GPU (tests/range_view_ref.py: scatter_reduce(amin) on int64 keys for the projection, nonzero + gather for the back-projection) and beside
the reference's numpy code on this box's CPU (oracle/range_view.py: the per-point Python loop that bench.py times as baseline B2, and the
vectorised numpy back-projection).
    python tools/time_range_view.py [--points 169600,2000000,8000000] [--loop-max-points N] [--json FILE]
169 600 points are one sweep (one per pixel); 2 M and 8 M are a map projected into a pose, about 12 and 47 contenders per pixel.  Device
times are device events around enough calls to fill --window seconds after a warm-up, three interleaved passes per leg, medians reported.
A call is what a user makes: the Python front with its output and scratch allocation (from torch's caching allocator) and its three
launches; for the back-projection it includes the one read of the count.  The projection's algorithmic traffic is 16 B read + one 8-B
atomic per point (+ 8 B fill, 8 B read and 8 B write per pixel): `native_gbps` is that over the call time.  No number here is a pass
criterion."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lidar-gs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import build_hip
import lidargs_scenes as sc
import range_view as rv
import range_view_ref as ref
from oracle import range_view as loop

ap = argparse.ArgumentParser()
ap.add_argument("--points", default="169600,2000000,8000000")
ap.add_argument("--loop-max-points", type=int, default=8000000, help="the numpy loop (about 3 s per million points) runs up to this many points")
ap.add_argument("--window", type=float, default=0.3, help="seconds of device work per timed window")
ap.add_argument("--json", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"
DEV = "cuda:0"
H, W = 64, 2650
beams = sc.beam_table(H, "waymo")
d_beams = torch.from_numpy(beams).to(DEV)


def timeit(fn):
    for _ in range(3):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(iters):
        torch.cuda.synchronize()
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / iters
    iters = max(5, min(2000, int(a.window * 1e3 / max(window(5), 1e-3))))
    return window(iters), iters


def legs_ms(legs):
    times = {k: [] for k in legs}
    iters = {}
    for _ in range(3):                                     # interleaved: every leg sees the same box state
        for k, fn in legs.items():
            t, iters[k] = timeit(fn)
            times[k].append(t)
    return {k: (statistics.median(v), [round(t, 4) for t in v], iters[k]) for k, v in times.items()}


res = dict(device=torch.cuda.get_device_name(0), box=build_hip.box_id(), build=build_hip.build_id(), image=[H, W], beam_table="waymo",
           window_s=a.window, projection=[], back_projection=None)
for N in (int(n) for n in a.points.split(",")):
    pts = ref.random_points(np.random.default_rng(N), N, beams, hi=85.0)
    d_pts = torch.from_numpy(pts).to(DEV)
    native = lambda: rv.lidar_to_pano_with_intensities(d_pts, H, W, beam_inclinations=d_beams)
    framework = lambda: ref.framework_project(d_pts, H, W, d_beams)
    n_p, n_i = native()
    f_p, f_i = framework()
    row = dict(points=N, contenders_per_pixel=round(float(N) / (H * W), 1), non_empty_pixels=int((n_p != 0).sum()),
               framework_differing_pixels=int((n_p != f_p).sum() + (n_i != f_i).sum()))
    for k, (ms, every, iters) in legs_ms(dict(native=native, framework=framework)).items():
        row[k + "_ms"], row[k + "_all"], row[k + "_iters"] = round(ms, 4), every, iters
    row["native_points_per_s"] = round(N / (row["native_ms"] * 1e-3))
    row["native_gbps"] = round((24.0 * N + 24.0 * H * W) / (row["native_ms"] * 1e-3) / 1e9, 1)
    if N <= a.loop_max_points:
        t0 = time.perf_counter()
        l_p, l_i = loop.points_to_pano(pts, H, W, beams)
        row["numpy_loop_s"] = round(time.perf_counter() - t0, 3)
        row["numpy_loop_points_per_s"] = round(N / row["numpy_loop_s"])
        row["numpy_loop_differing_pixels"] = int((n_p.cpu().numpy() != l_p).sum() + (n_i.cpu().numpy() != l_i).sum())     # unmasked points: a few may sit on a libm boundary
        row["native_speedup_over_numpy_loop"] = round(row["numpy_loop_s"] / (row["native_ms"] * 1e-3))
    res["projection"].append(row)
    print(f"project {N:8d} points: native {row['native_ms']:.4f} ms ({row['native_gbps']} GB/s of 24 B/point), framework ops {row['framework_ms']:.4f} ms"
          + (f", numpy loop {row['numpy_loop_s']:.2f} s ({row['numpy_loop_points_per_s']} points/s)" if "numpy_loop_s" in row else ""))
    del d_pts

pano = np.random.default_rng(1).uniform(3.0, 78.0, (H, W)).astype(np.float32)
inten = np.random.default_rng(2).uniform(0.0, 1.0, (H, W)).astype(np.float32)
d_pano, d_inten = torch.from_numpy(pano).to(DEV), torch.from_numpy(inten).to(DEV)
native = lambda: rv.pano_to_lidar_with_intensities(d_pano, d_inten, beam_inclinations=d_beams)
framework = lambda: ref.framework_unproject(d_pano, d_inten, d_beams)
row = dict(pixels=H * W, points=int(native().shape[0]),
           native_vs_framework_max_abs=float((native() - framework()).abs().max()))
for k, (ms, every, iters) in legs_ms(dict(native=native, framework=framework)).items():
    row[k + "_ms"], row[k + "_all"], row[k + "_iters"] = round(ms, 4), every, iters
ts = []
for _ in range(5):
    t0 = time.perf_counter()
    loop.pano_to_points(pano, inten, beams)
    ts.append(time.perf_counter() - t0)
row["numpy_ms"] = round(statistics.median(ts) * 1e3, 3)
res["back_projection"] = row
print(f"unproject {H}x{W} full image: native {row['native_ms']:.4f} ms, framework ops {row['framework_ms']:.4f} ms, numpy on the CPU {row['numpy_ms']:.2f} ms")
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
