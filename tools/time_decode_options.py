"""Time the anchor decode (forward + backward) with the two model options -- the feature bank and the appearance embedding -- against
the plain decode in the same run, and against the reference's chain of framework ops on the same GPU for each configuration.
    python tools/time_decode_options.py [--anchors N] [--k K] [--iters I] [--feat-bank 0|1] [--appearance-dim A] [--hip-only] [--json FILE]
Without --feat-bank / --appearance-dim all four configurations run (neither, bank, appearance 32, both), three interleaved passes
each, medians reported.  With them, that one configuration (what a kernel trace is taken of: --hip-only leaves the framework leg out).
Algorithmic bytes of the two bank kernels (140 + 128 and 268 + 140 per visible anchor) are printed with the visible count, for the
achieved bytes/s over a kernel time from a trace."""
import argparse, json, os, statistics, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lidar-gs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import lidargs_scenes as sc
import decode_options_ref as ref
from neural_gaussians import generate_neural_gaussians

ap = argparse.ArgumentParser()
ap.add_argument("--anchors", type=int, default=333_334)
ap.add_argument("--k", type=int, default=6)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--feat-bank", type=int, default=None)
ap.add_argument("--appearance-dim", type=int, default=None)
ap.add_argument("--hip-only", action="store_true")
ap.add_argument("--json", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"

base, cam, vis, _rng = sc.make_anchor_model(a.anchors, a.k, 5)
camera = types.SimpleNamespace(camera_center=torch.from_numpy(cam).cuda(), uid=1)
vmask = torch.from_numpy(vis).cuda()
if a.feat_bank is None and a.appearance_dim is None:
    configs = [("neither", False, 0), ("bank", True, 0), ("appearance32", False, 32), ("both", True, 32)]
else:
    configs = [("chosen", bool(a.feat_bank), int(a.appearance_dim or 0))]


def make(bank, A):
    p = ref.random_options(base, 5, bank=bank, A=A)
    pc = ref.to_torch_model(p)
    T = {n: t for n, t in (("anchor_feat", pc._anchor_feat), ("anchor", pc._anchor), ("offset", pc._offset), ("scaling", pc.get_scaling))}
    seqs = [(m, getattr(pc, "mlp_" + m)) for m in ref.MLPS] + ([("bank", pc.mlp_feature_bank)] if bank else [])
    for m, seq in seqs:
        T[m + "_W1"], T[m + "_b1"], T[m + "_W2"], T[m + "_b2"] = seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias
    if A:
        T["emb_color"], T["emb_raydrop"] = pc.get_appearance.weight, pc.get_appearance_rd.weight
    hip = lambda: generate_neural_gaussians(camera, pc, vmask, is_training=True)
    eager = lambda: ref.generate(T, camera.camera_center, vmask, ref.flags_of(p), camera.uid)
    return list(T.values()), hip, eager


def step(leaves, fn):
    for t in leaves:
        t.grad = None
    outs = fn()
    (outs[0].sum() + outs[1].sum() + outs[2].sum() + outs[3].sum() + outs[4].sum()).backward()
    return outs[0].shape[0]


def timeit(leaves, fn):
    for _ in range(3):
        step(leaves, fn)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(a.iters):
        step(leaves, fn)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / a.iters


built = {name: make(bank, A) for name, bank, A in configs}
times = {name: dict(hip=[], eager=[]) for name in built}
M = {name: step(b[0], b[1]) for name, b in built.items()}
for _ in range(3):                                        # interleaved: every configuration sees the same box state
    for name, (leaves, hip, eager) in built.items():
        times[name]["hip"].append(timeit(leaves, hip))
        if not a.hip_only:
            times[name]["eager"].append(timeit(leaves, eager))
n_vis = int(vis.sum())
res = dict(device=torch.cuda.get_device_name(0), anchors=a.anchors, k=a.k, visible=n_vis, iters=a.iters, rows=[],
           bank_forward_bytes=n_vis * (140 + 128), bank_backward_bytes=n_vis * (268 + 140))
for name, bank, A in configs:
    h = statistics.median(times[name]["hip"])
    e = statistics.median(times[name]["eager"]) if not a.hip_only else None
    res["rows"].append(dict(config=name, feat_bank=bank, appearance_dim=A, gaussians=M[name], hip_ms=round(h, 4), hip_all=[round(t, 4) for t in times[name]["hip"]],
                            framework_ms=None if e is None else round(e, 4)))
    print(f"decode N={a.anchors} k={a.k} {name:13s} (bank={int(bank)}, A={A:2d}): {M[name]} Gaussians; forward+backward HIP {h:.3f} ms"
          + ("" if e is None else f" vs framework ops {e:.3f} ms"))
print(f"visible anchors {n_vis}: bank forward {res['bank_forward_bytes'] / 1e6:.1f} MB, bank backward {res['bank_backward_bytes'] / 1e6:.1f} MB (algorithmic)")
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
