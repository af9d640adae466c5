"""What the pose gradient costs: one forward + backward of a BASELINE config through GaussianRasterizer with
`viewmatrix.requires_grad` off and on, alternated in one process (EXPERIMENTS.md).

    python tools/time_pose_grad.py [--config cfg3] [--rounds 5] [--steps 20] [--warmup 5] [--out FILE.json]
    python tools/time_pose_grad.py --surfel [...]      the surfel rasterizer on BASELINE config 5 (lgsfpose_backward_view)

Each round times `steps` frames without the request, then `steps` frames with it: a host clock around work that ends in a device
synchronise.  Prints the per-round times, the medians and their difference, and one JSON line; needs a HIP device.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lidar-gs_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=None, help="a BASELINE config (cfg3; with --surfel: cfg5)")
    ap.add_argument("--surfel", action="store_true", help="diff_lidargs_surfel_rasterization instead of diff_lidargs_rasterization")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_pose_grad: no HIP device; a time is measured on the GPU or not at all")
    import lidargs_scenes as sc
    a.config = a.config or ("cfg5" if a.surfel else "cfg3")
    kind, P, H, W, seed = sc.BASELINE_CONFIGS[a.config]
    scene = sc.make_scene(kind, P, H, seed)
    if a.surfel:
        import numpy as np
        from diff_lidargs_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
        from util import surfel_upstream_grads
        scene["scales"] = np.ascontiguousarray(scene["scales"][:, :2])
        upstream = surfel_upstream_grads(H, W, seed)                    # (colour [2,H,W], others [7,H,W]: bench.py's cfg5 cotangents)
        settings = lambda s: GaussianRasterizationSettings(
            image_height=H, image_width=W, bg=s["bg"], scale_modifier=1.0, depth_threshold=0.0, viewmatrix=s["viewmatrix"],
            projmatrix=torch.eye(4, device="cuda"), sh_degree=1, campos=torch.zeros(3, device="cuda"), prefiltered=False,
            beam_inclinations=s["beams"], lidar_far=80, lidar_near=0, debug=False)
        planes = lambda out: [out[0], out[2]]                           # (color, radii, others, pixels)
    else:
        from diff_lidargs_rasterization import GaussianRasterizer
        upstream = sc.upstream_grads(H, W, seed)
        settings = lambda s: sc.raster_settings(s, W, H)
        planes = lambda out: list(out[:3])                              # (color, depth, occ, radii)
    st = {k: torch.from_numpy(v).cuda() for k, v in scene.items()}
    leaves = [st[k].clone().requires_grad_(True) for k in ("means3D", "colors", "opacities", "scales", "rotations")]
    m2 = torch.zeros(P, 4, device="cuda", requires_grad=True)
    g = [torch.from_numpy(x).cuda() for x in upstream]
    rast = {}
    for pose in (False, True):
        vm = st["viewmatrix"].clone().requires_grad_(pose)
        rast[pose] = (GaussianRasterizer(settings(dict(st, viewmatrix=vm))), vm)

    def step(pose):
        r, vm = rast[pose]
        out = r(means3D=leaves[0], means2D=m2, opacities=leaves[2], colors_precomp=leaves[1], scales=leaves[3], rotations=leaves[4])
        torch.autograd.backward(planes(out), g)
        for t in leaves + [m2, vm]:
            t.grad = None

    def timed(pose, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step(pose)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for pose in (False, True):
        timed(pose, a.warmup)
    ms = {False: [], True: []}
    for r in range(a.rounds):
        for pose in (False, True):
            ms[pose].append(timed(pose, a.steps))
        print(f"round {r}: without {ms[False][-1]:.4f} ms/frame, with {ms[True][-1]:.4f} ms/frame")
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    res = dict(tool="time_pose_grad", rasterizer="surfel" if a.surfel else "3d", config=a.config, P=P, H=H, W=W, rounds=a.rounds, steps=a.steps, ms_without=ms[False], ms_with=ms[True],
               median_ms_without=off, median_ms_with=on, median_extra_ms=on - off,
               spread_ms_without=max(ms[False]) - min(ms[False]), spread_ms_with=max(ms[True]) - min(ms[True]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
