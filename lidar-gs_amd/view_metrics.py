"""The per-view metric block of training_report (the reference's train.py:314-377) on the device.

`view_metrics(render, depth, gt_image, ...)` returns, for one rendered view, the 11 values of the reference's log line (train.py:378) as
one float64 device tensor -- L1, PSNR, SSIM, intensity MAE, RMSE, MedAE, chamfer distance, F-score, depth MAE, MedAE, RMSE -- from ONE
native call (include/lidargs_metrics.h lidargs_view_metrics).  The reference copies the image and its ground truth to the host for
scikit-image's structural_similarity, takes two torch medians and reads the points meter's result back for every view; here nothing is
read back.  The SSIM restates scikit-image's default algorithm from its publication; it is not pinned against scikit-image itself.

`ViewMeter` collects one row per view and reads them back once, in `measure()`."""
import numpy as np
import torch

from diff_lidargs_rasterization import _C as _base

_lib = _base._lib

NAMES = ("l1", "psnr", "ssim", "in_mae", "in_rmse", "in_medae", "cd", "fscore", "mae", "medae", "rmse")


def _beams_on(beam_inclinations, dev, H):
    if torch.is_tensor(beam_inclinations) and beam_inclinations.is_cuda:
        beams = beam_inclinations.detach().to(dev, torch.float32).contiguous()
    else:
        b = beam_inclinations.detach().cpu().numpy() if torch.is_tensor(beam_inclinations) else np.asarray(beam_inclinations)
        beams = torch.as_tensor(b, dtype=torch.float32).to(dev).contiguous()
    if beams.numel() != H:
        raise RuntimeError("view_metrics: beam_inclinations must have one entry per image row")
    return beams


def view_metrics(render, depth, gt_image, beam_inclinations=None, intrinsics=None, depth_min=5.0, depth_max=80.0, out=None,
                 points_meter=True):
    """render f32[2, H, W] (intensity, ray-drop), depth f32[1, H, W], gt_image f32[3, H, W] (ray-drop mask, intensity, depth), all on a
    HIP device; beam_inclinations [H] (ascending) or intrinsics = (fov_up, fov) in degrees; depth_min / depth_max as opt.depth_min /
    opt.depth_max.  -> float64[11] on the device (NAMES), written into `out` when given.  points_meter=False skips the chamfer /
    F-score part (slots 6 and 7 are NaN)."""
    _base._require_device(render, "render"); _base._require_device(depth, "depth"); _base._require_device(gt_image, "gt_image")
    if render.ndim != 3 or render.shape[0] != 2:
        raise RuntimeError("view_metrics: render must be [2, H, W] (intensity, ray-drop)")
    H, W = int(render.shape[1]), int(render.shape[2])
    if tuple(depth.shape) != (1, H, W) or tuple(gt_image.shape) != (3, H, W):
        raise RuntimeError("view_metrics: depth must be [1, H, W] and gt_image [3, H, W] of the render's H, W")
    if H < 7 or W < 7:
        raise RuntimeError("view_metrics: the SSIM's 7 x 7 window needs H >= 7 and W >= 7")
    dev = render.device
    if depth.device != dev or gt_image.device != dev:
        raise RuntimeError("view_metrics: all inputs must be on one device")
    p32 = lambda t: t.detach().to(torch.float32).contiguous()
    render, depth, gt_image = p32(render), p32(depth), p32(gt_image)
    beams = None
    fov_up = fov = 0.0
    if points_meter:
        if beam_inclinations is not None:
            beams = _beams_on(beam_inclinations, dev, H)
        elif intrinsics is not None:
            fov_up, fov = float(intrinsics[0]), float(intrinsics[1])
        else:
            raise RuntimeError("view_metrics: need beam_inclinations or intrinsics = (fov_up, fov)")
    if out is None:
        out = torch.empty(11, dtype=torch.float64, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float64 and out.numel() == 11 and out.is_contiguous()):
        raise RuntimeError("view_metrics: out must be a contiguous float64[11] tensor on the inputs' device")
    nb = _lib.lidargs_view_metrics_scratch_bytes(H, W)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lidargs_view_metrics_ex(H, W, _base._ptr(render), _base._ptr(depth), _base._ptr(gt_image), float(depth_min),
                                          float(depth_max), _base._ptr(beams), fov_up, fov, 1 if points_meter else 0, _base._ptr(out),
                                          _base._ptr(scratch), nb, _base._stream(dev))
    if rc < 0:
        _base._raise(rc, "view_metrics")
    return out


class ViewMeter:
    """The accumulators of training_report (train.py:301-312, :341-371) for one camera set: update() per view keeps the view's row on
    the device, measure() reads them back once and returns the 11 means over the views (what the reference divides by
    len(config['cameras']), :376-386) as float64 numpy, in NAMES order."""

    def __init__(self, depth_min, depth_max):
        self.depth_min = depth_min
        self.depth_max = depth_max
        self.rows = []

    def clear(self):
        self.rows = []

    def update(self, render, depth, gt_image, beam_inclinations):
        self.rows.append(view_metrics(render, depth, gt_image, beam_inclinations=beam_inclinations, depth_min=self.depth_min,
                                      depth_max=self.depth_max))

    def measure(self):
        if not self.rows:
            return np.full(len(NAMES), np.nan)
        return torch.stack(self.rows).mean(0).cpu().numpy()
