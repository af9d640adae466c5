"""Time one optimizer step of the bench's decode model (333 334 anchors x 6 offsets, four MLPs: lidargs_scenes.make_anchor_model as
`bench.py --workload decode` builds it) with lidargs_optim.Adam and with torch.optim.Adam's three device paths, in one process,
alternating the four in rounds.  The groups are the training script's ten (scene/gaussian_model.py:372-388): anchor, offset,
anchor_feat, opacity, scaling, rotation and the four MLPs; opacity and rotation never have a gradient.  Gradients are filled once.

    python tools/time_adam.py [--steps 300] [--warmup 20] [--rounds 3] [--host-reps 200] [--only ours] [--out FILE.json]

Per path:
  device_us   HIP events around `--steps` back-to-back step() calls after `--warmup`, divided by the steps (the median of the rounds):
              the time the stream is busy per step; where the host cannot keep the queue filled this is the host's pace
  host_us     time.perf_counter() around ONE step() call with the queue empty (a synchronise before each call, outside the clock):
              what the call costs the training loop's thread; median of `--host-reps`
  bytes_per_s 28 bytes (four float32 loads, three stores) per element that has a gradient, over device_us
`--only NAME` runs one path alone (for a `rocprofv3 --kernel-trace --stats` run, which shows the launches per step)."""
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
from torch import nn  # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12      # float4 copy on this part
BYTES_PER_ELEMENT = 28


def build_groups(N, k, seed):
    import lidargs_scenes as sc
    p, _cam, _vis, rng = sc.make_anchor_model(N, k, seed)
    pc = sc.anchor_model_to_torch(p)
    leaf = lambda t: nn.Parameter(t.detach().clone())
    dev = pc._anchor.device
    groups = [{"params": [leaf(pc._anchor)], "lr": 0.0, "name": "anchor"},
              {"params": [leaf(pc._offset)], "lr": 0.01, "name": "offset"},
              {"params": [leaf(pc._anchor_feat)], "lr": 0.0075, "name": "anchor_feat"},
              {"params": [nn.Parameter(torch.zeros(N, 1, device=dev))], "lr": 0.02, "name": "opacity"},
              {"params": [leaf(pc.get_scaling)], "lr": 0.007, "name": "scaling"},
              {"params": [nn.Parameter(torch.zeros(N, 4, device=dev))], "lr": 0.002, "name": "rotation"}]
    for name, lr in (("opacity", 0.002), ("cov", 0.004), ("color", 0.008), ("raydrop", 0.008)):
        groups.append({"params": [leaf(t) for t in getattr(pc, "mlp_" + name).parameters()], "lr": lr, "name": "mlp_" + name})
    gen = torch.Generator(device=dev).manual_seed(seed + 1)
    for g in groups:
        if g["name"] in ("opacity", "rotation"):
            continue
        for q in g["params"]:
            q.grad = 1e-3 * torch.randn(q.shape, device=dev, generator=gen)
    return groups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, default=333_334)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=200)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    import build_hip
    build_hip.build()
    from lidargs_optim import Adam
    kw = dict(lr=0.0, eps=1e-15)
    makers = {"ours": lambda g: Adam(g, **kw),
              "torch foreach=False": lambda g: torch.optim.Adam(g, foreach=False, fused=False, **kw),
              "torch foreach=True": lambda g: torch.optim.Adam(g, foreach=True, **kw),
              "torch fused=True": lambda g: torch.optim.Adam(g, fused=True, **kw)}
    if a.only:
        makers = {a.only: makers[a.only]}
    opts, elements, tensors = {}, 0, 0
    for name, make in makers.items():
        groups = build_groups(a.anchors, 6, 5)
        elements = sum(q.numel() for g in groups for q in g["params"] if q.grad is not None)
        tensors = sum(1 for g in groups for q in g["params"] if q.grad is not None)
        opts[name] = make(groups)
    for opt in opts.values():
        for _ in range(a.warmup):
            opt.step()
    torch.cuda.synchronize()
    dev_us = {n: [] for n in opts}
    for _ in range(a.rounds):
        for name, opt in opts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                opt.step()
            e1.record()
            torch.cuda.synchronize()
            dev_us[name].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    host_us = {n: [] for n in opts}
    for _ in range(a.host_reps):
        for name, opt in opts.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter(); opt.step(); host_us[name].append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    res = dict(device=torch.cuda.get_device_name(0), box=build_hip.box_id(), build=build_hip.build_id(), torch=torch.__version__, anchors=a.anchors,
               tensors_with_gradient=tensors, elements=elements, bytes_per_step=elements * BYTES_PER_ELEMENT,
               floor_us_at_6_29_TB_s=elements * BYTES_PER_ELEMENT / HBM_COPY_BYTES_PER_S * 1e6, steps=a.steps, warmup=a.warmup, rounds=a.rounds,
               host_reps=a.host_reps, rows=[])
    for name in opts:
        d = float(np.median(dev_us[name]))
        row = dict(path=name, device_us=d, device_us_rounds=[round(x, 2) for x in dev_us[name]], host_us=float(np.median(host_us[name])),
                   host_us_min=float(min(host_us[name])), bytes_per_s=elements * BYTES_PER_ELEMENT / (d * 1e-6),
                   share_of_copy_rate=elements * BYTES_PER_ELEMENT / (d * 1e-6) / HBM_COPY_BYTES_PER_S)
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
    if len(opts) > 1:
        best_dev = min(r["device_us"] for r in res["rows"] if r["path"] != "ours")
        best_host = min(r["host_us"] for r in res["rows"] if r["path"] != "ours")
        ours = res["rows"][0]
        res["ours_not_slower_on_device"] = bool(ours["device_us"] <= best_dev)
        res["ours_not_slower_on_host"] = bool(ours["host_us"] <= best_host)
        print(json.dumps({k: res[k] for k in ("elements", "floor_us_at_6_29_TB_s", "ours_not_slower_on_device", "ours_not_slower_on_host")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
