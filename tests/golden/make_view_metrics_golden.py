"""Generate tests/golden/view_metrics_golden.npz by EXECUTING the reference's per-view metric block of training_report
(train.py:314-371, the loop over the cameras) on CPU torch.

Run in the authoring container only (needs /root/reference):

    python tests/golden/make_view_metrics_golden.py

Executed reference code (nothing of its source text is written to this repository; the .npz holds inputs and outputs only):
  the `for idx, viewpoint in enumerate(config['cameras'])` loop of training_report   train.py:314-371   (pulled out of the file's AST:
                                                                                      the module itself cannot be imported here)
  l1_loss                                                                            utils/loss_utils.py   (executed as it stands)
  psnr                                                                               utils/image_utils.py  (executed as it stands)
Stand-ins, stated:
  structural_similarity   tests/view_metrics_ref.ssim, the restatement of scikit-image's default algorithm (scikit-image is not installed)
  PointsMeter             oracle/points_meter.update on the two [H, W] images (the fixture path of tests/test_points_meter.py)
  prefilter_voxel, renderFunc, the camera   return the case's render / depth / ground truth; tb_writer is None (no images)
One camera per run, so each accumulator holds that view's value.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]
import view_metrics_ref as R  # noqa: E402
from oracle import points_meter as pm_oracle  # noqa: E402

REF = "/root/reference"
ACC = ("l1_test", "psnr_test", "in_ssim", "in_mae", "in_rmse", "in_medae", "cd_test", "fscore_test", "mae", "medae", "rmse")


def camera_loop():
    src = os.path.join(REF, "train.py")
    tree = ast.parse(open(src).read(), src)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "training_report")
    loops = [n for n in ast.walk(fn) if isinstance(n, ast.For) and isinstance(n.target, ast.Tuple)
             and [e.id for e in n.target.elts] == ["idx", "viewpoint"]]
    assert len(loops) == 1
    return compile(ast.Module(body=loops, type_ignores=[]), src, "exec")


def helpers():
    ns = {"torch": torch}
    for f in ("utils/loss_utils.py", "utils/image_utils.py"):
        p = os.path.join(REF, f)
        tree = ast.parse(open(p).read(), p)
        body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("l1_loss", "psnr")]
        exec(compile(ast.Module(body=body, type_ignores=[]), p, "exec"), ns)
    return ns["l1_loss"], ns["psnr"]


class _OnHost:
    """original_image.cuda() on a host without a device: the tensor itself."""
    def __init__(self, t):
        self.t = t

    def cuda(self):
        return self.t


class _PointsMeter:
    def __init__(self, scale, intrinsics, beam_inclinations):
        self.beams, self.scale, self.v = beam_inclinations, scale, None

    def update(self, preds, truths):
        cd, f, *_ = pm_oracle.update(preds[0].numpy(), truths[0].numpy(), self.beams, self.scale)
        self.v = np.array([cd, f], np.float32)

    def measure(self):
        return self.v


def run_reference(code, l1_loss, psnr, render, depth, gt, beams, dmin, dmax):
    cam = types.SimpleNamespace(original_image=_OnHost(torch.from_numpy(gt)), beam_inclinations=torch.from_numpy(beams), image_name="v")
    pkg = {"render": torch.from_numpy(render), "depth": torch.from_numpy(depth)}
    ns = dict(torch=torch, np=np, config={"cameras": [cam], "name": "test"}, scene=types.SimpleNamespace(gaussians=None), renderArgs=(),
              prefilter_voxel=lambda *a, **k: None, renderFunc=lambda *a, **k: pkg, tb_writer=None,
              opt=types.SimpleNamespace(depth_min=dmin, depth_max=dmax), l1_loss=l1_loss, psnr=psnr,
              structural_similarity=lambda a, b, data_range: R.ssim(a, b) if data_range == 1.0 else None, PointsMeter=_PointsMeter)
    ns.update({k: 0.0 for k in ACC})
    exec(code, ns)
    return np.array([float(ns[k]) for k in ACC], np.float64)


def make_case(rng, H, W, kind):
    import lidargs_scenes as sc
    depth = rng.gamma(2.0, 12.0, size=(1, H, W)).astype(np.float32) + 1.0
    gt_mask = (rng.random((H, W)) > 0.15).astype(np.float32)
    gt_int = rng.beta(2.0, 5.0, size=(H, W)).astype(np.float32)
    gt_depth = (depth[0] * (1.0 + 0.02 * rng.normal(size=(H, W)))).astype(np.float32)
    gt = np.stack([gt_mask, gt_int, gt_depth]).astype(np.float32)
    inten = (gt_int + 0.1 * rng.normal(size=(H, W))).astype(np.float32)           # some below 0 and above 1: the clamp
    drop = (gt_mask * 0.8 + 0.3 * rng.random((H, W))).astype(np.float32)
    if kind == "edges":
        drop.flat[rng.choice(H * W, H * W // 10, replace=False)] = 0.5            # exactly 0.5: dropped (strict >)
        inten.flat[rng.choice(H * W, H * W // 10, replace=False)] = 1.5
        inten[gt_mask == 0] = 0.0
    if kind == "nan":
        inten[2, 3] = np.nan                                                       # NaN survives the clamp and the mask
    if kind == "ties":
        z = rng.random((H, W)) < 0.7
        inten[z] = 0.0; gt[1][z] = 0.0; drop[z] = 0.9
        depth[0][z] = 5.0; gt[2][z] = 5.0; gt[0][z] = 1.0
    render = np.stack([inten, drop]).astype(np.float32)
    beams = np.ascontiguousarray(sc.beam_table(H, "waymo"), dtype=np.float32)
    return render, depth, gt, beams


def main():
    sys.path.insert(0, os.path.join(HERE, "..", "..", "lidar-gs_amd"))
    code = camera_loop()
    l1_loss, psnr = helpers()
    out = {}
    cases = {"a": (16, 96, "plain", 31), "b": (9, 40, "edges", 32), "c": (8, 33, "nan", 33), "d": (12, 64, "ties", 34), "e": (7, 7, "plain", 35)}
    dmin, dmax = 5.0, 80.0
    for tag, (H, W, kind, seed) in cases.items():
        rng = np.random.default_rng(seed)
        render, depth, gt, beams = make_case(rng, H, W, kind)
        v = run_reference(code, l1_loss, psnr, render, depth, gt, beams, dmin, dmax)
        out.update({f"{tag}_render": render, f"{tag}_depth": depth, f"{tag}_gt": gt, f"{tag}_beams": beams, f"{tag}_out": v,
                    f"{tag}_depth_range": np.array([dmin, dmax], np.float32)})
        print(tag, H, W, kind, v)
    dst = os.path.join(HERE, "view_metrics_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
