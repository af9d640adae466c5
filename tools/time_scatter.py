"""Device time of the torch_scatter stand-in's scatter_max (lidar-gs_amd/torch_scatter/) on a shape like the reference's call
(scene/gaussian_model.py:742: candidate features [rows, 32] into about a third as many voxels, index `inv.unsqueeze(1).expand(-1, 32)`),
beside torch's own device op on the same GPU: torch.zeros(...).scatter_reduce_(0, idx, src, "amax", include_self=False).
    python tools/time_scatter.py [--rows 2000000] [--cols 32] [--once] [--json FILE]
Two legs each: the forward alone, and the forward plus the backward of `out.sum()`-like upstream gradient (a fixed grad_out).  torch's op
gives no `arg` and splits the gradient among ties, so it is the yardstick for time only.  Device events around enough calls to fill
--window seconds after a warm-up, three interleaved passes per leg, medians reported.  A call is what a user makes: the Python front with
its checks (the one host read of the index's range included), its output and scratch allocation and its launches.  The forward's
algorithmic traffic is 4 B of src per element (the index is 8 B per ROW, broadcast), one 8-B atomic per element, and 8 B fill + 8 B read +
12 B write per output element.  `--once` makes one call of every leg and times nothing: the run to put under a kernel trace.  No number
here is a pass criterion."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lidar-gs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import build_hip
from torch_scatter import scatter_max

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2000000)
ap.add_argument("--cols", type=int, default=32)
ap.add_argument("--window", type=float, default=0.3, help="seconds of device work per timed window")
ap.add_argument("--once", action="store_true", help="one call of every leg and no timing (for a kernel trace)")
ap.add_argument("--json", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"
DEV = "cuda:0"
N, F = a.rows, a.cols
G = max(1, N // 3)
g = torch.Generator().manual_seed(742)
src = torch.randn(N, F, generator=g).to(DEV)
inv = torch.randint(0, G, (N,), generator=g)
inv[:G] = torch.arange(G)                                   # every group has a member, as after torch.unique
inv = inv.to(DEV)
idx = inv.unsqueeze(1).expand(-1, F)                        # stride (1, 0): the reference's form
grad_out = torch.randn(G, F, generator=g).to(DEV)
src_g = src.clone().requires_grad_()


def native_fwd():
    return scatter_max(src, idx, dim=0)[0]


def torch_fwd():
    return torch.zeros(G, F, device=DEV).scatter_reduce_(0, idx, src, "amax", include_self=False)


def native_fwd_bwd():
    src_g.grad = None
    scatter_max(src_g, idx, dim=0)[0].backward(grad_out)
    return src_g.grad


def torch_fwd_bwd():
    src_g.grad = None
    torch.zeros(G, F, device=DEV).scatter_reduce(0, idx, src_g, "amax", include_self=False).backward(grad_out)
    return src_g.grad


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


legs = dict(native_forward=native_fwd, torch_forward=torch_fwd, native_forward_backward=native_fwd_bwd, torch_forward_backward=torch_fwd_bwd)
same = bool(torch.equal(native_fwd().view(torch.int32), torch_fwd().view(torch.int32)))
res = dict(device=torch.cuda.get_device_name(0), box=build_hip.box_id(), build=build_hip.build_id(), rows=N, cols=F, groups=G,
           index="int64 [rows] expanded to [rows, cols] with stride (1, 0)", window_s=a.window, values_equal_torch_bit_for_bit=same)
if a.once:
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    print("one call of every leg; values equal torch's bit for bit:", same)
    sys.exit(0)
times, iters = {k: [] for k in legs}, {}
for _ in range(3):                                          # interleaved: every leg sees the same box state
    for k, fn in legs.items():
        t, iters[k] = timeit(fn)
        times[k].append(t)
for k, v in times.items():
    res[k + "_ms"], res[k + "_all"], res[k + "_iters"] = round(statistics.median(v), 4), [round(t, 4) for t in v], iters[k]
bytes_fwd = 4.0 * N * F + 8.0 * N + 8.0 * N * F + 28.0 * G * F
res["native_forward_gbps"] = round(bytes_fwd / (res["native_forward_ms"] * 1e-3) / 1e9, 1)
res["native_over_torch_forward"] = round(res["native_forward_ms"] / res["torch_forward_ms"], 3)
res["native_over_torch_forward_backward"] = round(res["native_forward_backward_ms"] / res["torch_forward_backward_ms"], 3)
print(f"scatter_max {N} x {F} into {G} groups (values equal torch's bit for bit: {same}), box {res['box']}, build {res['build']}")
print(f"  forward            native {res['native_forward_ms']:.4f} ms ({res['native_forward_gbps']} GB/s of its algorithmic bytes), "
      f"torch scatter_reduce_(amax) {res['torch_forward_ms']:.4f} ms")
print(f"  forward + backward native {res['native_forward_backward_ms']:.4f} ms, torch {res['torch_forward_backward_ms']:.4f} ms")
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
