"""Time the sweep-motion compensation (lidar-gs_amd/sweep_motion.py) against the same definition as float32 framework ops on the same GPU.

    python tools/time_sweep_motion.py [--points 2000000] [--iterations 3] [--rounds 5] [--window 0.3] [--out profiles/sweep_motion_time.json]

Four contenders -- native forward, framework forward (no_grad), native forward + backward (all three gradients), framework forward +
backward -- are warmed up and then timed in alternation: every round times each of them once over a window of `--window` seconds (a host
clock around work that ends in a device synchronise), and the figure reported per contender is the median of its rounds, with every round
listed.  The framework chain is tests/sweep_ref.py run on float32 device tensors: the closed-form exponential, the iterates with the seam
rule, autograd for the gradients.  Algorithmic bytes: 24 B per Gaussian forward (one 12-byte row in, one out); forward + backward 60 B
(the forward's 24, then two rows in and one out) plus one 128-byte partial row per 256 Gaussians, written and read once.

Not a test and no time is a criterion: the numbers are written down as measured.  Needs a HIP device."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lidar-gs_amd"), os.path.join(ROOT, "tests")]

import numpy as np
import torch


def timed(fn, window):
    """(milliseconds per call, calls) over at least `window` seconds."""
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    iters = max(3, int(window / max(time.perf_counter() - t0, 1e-6)))
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_motion_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sweep_motion: needs a HIP device (there is no CPU path to time)")
    import build_hip
    build_hip.build()
    import lidargs_scenes as sc
    import sweep_motion
    import sweep_ref as R

    P, n, sweep = a.points, a.iterations, (-0.5, 0.5)
    vm64 = torch.from_numpy(sc.rigid_viewmatrix(np.random.default_rng(18))).double()
    x = R.world_points(R.points(P, 1), vm64).float().cuda()
    vm, xi = vm64.float().cuda(), torch.tensor(R.TWIST, device="cuda")
    g = torch.randn(P, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    leaves = [t.clone().requires_grad_(True) for t in (x, vm, xi)]

    def native_fwd():
        with torch.no_grad():
            return sweep_motion.compensate(x, vm, xi, sweep, n)

    def chain_fwd():
        with torch.no_grad():
            return R.compensate(x, vm, xi, sweep, n)

    def both(fn):
        def step():
            for t in leaves:
                t.grad = None
            fn(*leaves, sweep, n).backward(g)
            return [t.grad for t in leaves]
        return step

    contenders = {"native_forward": native_fwd, "framework_forward": chain_fwd,
                  "native_forward_backward": both(sweep_motion.compensate), "framework_forward_backward": both(R.compensate)}
    # same inputs, same outputs: the largest differences between the two paths at the size that is timed
    d_out = float((native_fwd() - chain_fwd()).abs().max())
    gn, gf = contenders["native_forward_backward"](), contenders["framework_forward_backward"]()
    d_grads = [float((p - q).abs().max() / q.abs().max()) for p, q in zip([t.clone() for t in gn], gf)]
    for fn in contenders.values():                                     # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in contenders}
    for _ in range(a.rounds):                                          # alternated: one window each per round
        for k, fn in contenders.items():
            runs[k].append(timed(fn, a.window))
    res = dict(device=torch.cuda.get_device_name(0), box=build_hip.box_id(), build=build_hip.build_id(), points=P, iterations=n, sweep=sweep,
               twist=list(R.TWIST), window_s=a.window, rounds=a.rounds,
               max_abs_difference_x=d_out, max_difference_gradients_relative_to_largest=dict(zip(("means3D", "viewmatrix", "twist"), d_grads)))
    bytes_of = dict(native_forward=24 * P, native_forward_backward=60 * P + 2 * 128 * ((P + 255) // 256))
    for k, r in runs.items():
        ms = statistics.median(t for t, _ in r)
        res[k] = dict(ms=round(ms, 4), all_ms=[round(t, 4) for t, _ in r], iters=[i for _, i in r])
        if k in bytes_of:
            res[k].update(algorithmic_bytes=bytes_of[k], gbps=round(bytes_of[k] / ms / 1e6, 1))
    res["forward_speedup"] = round(res["framework_forward"]["ms"] / res["native_forward"]["ms"], 2)
    res["forward_backward_speedup"] = round(res["framework_forward_backward"]["ms"] / res["native_forward_backward"]["ms"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    print(f"sweep-motion compensation, {P} Gaussians, {n} iterations: forward {res['native_forward']['ms']:.4f} ms "
          f"({res['native_forward']['gbps']} GB/s of 24 B per Gaussian; framework ops {res['framework_forward']['ms']:.3f} ms), forward + backward "
          f"{res['native_forward_backward']['ms']:.4f} ms (framework ops {res['framework_forward_backward']['ms']:.3f} ms)")


if __name__ == "__main__":
    main()
