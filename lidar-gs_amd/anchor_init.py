"""`GaussianModel.voxelize_sample` of LiDAR-GS (the reference's scene/gaussian_model.py:272-276) on the native call of
include/lidargs_knn.h.

    from anchor_init import voxelize_sample
    points = voxelize_sample(points, voxel_size=gaussians.voxel_size)      # in create_from_pcd (:293)

The reference shuffles `data` in place with the global numpy generator and returns np.unique(np.round(data / voxel_size), axis=0) *
voxel_size.  Here, for a numpy array, the same shuffle runs (same draws, same side effect); the rounding, the sort and the unique run
on the current HIP device and a numpy array of the same dtype and rows comes back.  A tensor on a HIP device gives a tensor on it (no
shuffle: a shuffle changes nothing but which of -0.0 / +0.0 numpy keeps).  The arithmetic is the reference's in the precision numpy
picks for `data / voxel_size` (float32 data and a Python float stay float32 under NumPy 2; float64 stays float64).  Non-finite rows,
quotients of magnitude 2^62 and beyond, and voxel_size <= 0 raise RuntimeError.  There is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from diff_lidargs_rasterization import _C as _base

_lib = _base._lib


def voxelize_device(points, voxel_size):
    """points: float32 or float64 [P, 3] on a HIP device -> the distinct rows of round(points / voxel_size) * voxel_size in lexicographic
    order, same dtype and device (voxel_size is rounded to that dtype, as numpy does for a Python float)."""
    _base._require_device(points, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f"voxelize_sample: `points` must have shape [P, 3], got {list(points.shape)}")
    if points.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"voxelize_sample: `points` must be float32 or float64, got {points.dtype}")
    v = float(voxel_size)
    if not (v > 0.0):
        raise RuntimeError(f"voxelize_sample: voxel_size must be positive, got {voxel_size}")
    pts = points.detach().contiguous()
    P, dev, dt = int(pts.shape[0]), pts.device, pts.dtype
    if P == 0:
        return torch.empty((0, 3), dtype=dt, device=dev)
    nb = _lib.lidargs_voxelize_scratch_bytes(P)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    out = _base._Scratch(dev)
    with torch.cuda.device(dev):
        rc = _lib.lidargs_voxelize_sample(P, C.c_void_p(pts.data_ptr()), 1 if dt == torch.float64 else 0, v,
                                          _base._ptr(scratch), nb, out.cb, out.user, _base._stream(dev))
    t = out.take()
    if rc < 0:
        _base._raise(rc, "voxelize_sample")
    return t[: rc * 3 * pts.element_size()].view(dt).view(rc, 3)


def voxelize_sample(data=None, voxel_size=0.01):
    """Drop-in for GaussianModel.voxelize_sample(data, voxel_size) (numpy in, numpy out, shuffling `data` in place first), or the same
    on a device tensor."""
    if isinstance(data, torch.Tensor):
        return voxelize_device(data, voxel_size)
    np.random.shuffle(data)                                            # :273 -- the global generator's draws and the in-place side effect
    dt = (np.empty((0, 3), dtype=np.asarray(data).dtype) / voxel_size).dtype    # the dtype numpy computes data / voxel_size in
    if dt not in (np.float32, np.float64):
        raise RuntimeError(f"voxelize_sample: data / voxel_size is {dt}; only float32 and float64 are supported")
    arr = np.ascontiguousarray(np.asarray(data, dtype=dt))
    if arr.ndim != 2 or arr.shape[1] != 3:
        raise RuntimeError(f"voxelize_sample: `data` must have shape [P, 3], got {list(arr.shape)}")
    if not torch.cuda.is_available():
        raise RuntimeError("voxelize_sample: needs a HIP device; there is no CPU path")
    v = float(np.asarray(voxel_size, dtype=np.float64))
    res = voxelize_device(torch.from_numpy(arr).cuda(), v)
    return res.cpu().numpy()
