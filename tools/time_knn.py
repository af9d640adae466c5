"""Time the model-initialisation kernels of include/lidargs_knn.h on the accumulated scan (lidargs_scenes.accumulated_scan):
distCUDA2 at 1, 4 and 16 M points and voxelize_sample at 4 M, next to scipy's cKDTree (16 threads) and np.unique on the host.

    python tools/time_knn.py [--sizes 1,4,16] [--reps 10] [--warmup 2] [--cpu-reps 1] [--out FILE.json]

GPU numbers: median of `--reps` timed calls after `--warmup`, each bracketed by torch.cuda.synchronize() (wall clock, includes the
Python wrapper, the scratch allocation and for voxelize_sample its two host reads).  Host numbers: median of `--cpu-reps` runs."""
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


def _cpu_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4,16")
    ap.add_argument("--voxel-size", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None, help="also write the rows as JSON here")
    a = ap.parse_args()
    import build_hip
    build_hip.build()
    import lidargs_scenes as sc
    from simple_knn._C import distCUDA2
    from anchor_init import voxelize_sample
    res = dict(device=torch.cuda.get_device_name(0), build=build_hip.build_id(), reps=a.reps, warmup=a.warmup, cpu_reps=a.cpu_reps, knn=[], voxelize=[])
    for m in [int(s) for s in a.sizes.split(",")]:
        P = m << 20
        x = sc.accumulated_scan(P, 1)
        xd = torch.from_numpy(x).cuda()
        med, lo, hi = _gpu_ms(lambda: distCUDA2(xd), a.reps, a.warmup)
        row = dict(P=P, gpu_ms=med, gpu_min_ms=lo, gpu_max_ms=hi, ns_per_point=med * 1e6 / P)
        if not a.no_cpu:
            from scipy.spatial import cKDTree
            x64 = x[np.isfinite(x).all(1)].astype(np.float64)
            row["ckdtree_ms"] = _cpu_ms(lambda: cKDTree(x64).query(x64, k=4, workers=16), a.cpu_reps)
        print(json.dumps(row), flush=True)
        res["knn"].append(row)
        if m == a.voxel_size:
            d = distCUDA2(xd)
            v = torch.kthvalue(d, int(P * 0.5))[0].item()
            med, lo, hi = _gpu_ms(lambda: voxelize_sample(xd, v), a.reps, a.warmup)
            U = int(voxelize_sample(xd, v).shape[0])
            row = dict(P=P, voxel_size=v, U=U, gpu_ms=med, gpu_min_ms=lo, gpu_max_ms=hi)
            xn = x.copy()
            row["numpy_path_ms"] = _cpu_ms(lambda: voxelize_sample(xn, v), max(1, a.cpu_reps))      # shuffle + upload + device + download
            if not a.no_cpu:
                row["np_unique_ms"] = _cpu_ms(lambda: np.unique(np.round(xn / v), axis=0) * v, a.cpu_reps)
            print(json.dumps(row), flush=True)
            res["voxelize"].append(row)
        del xd
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
