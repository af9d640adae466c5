"""`simple_knn._C.distCUDA2` on the native call of include/lidargs_knn.h (csrc/knn.hip).

    from simple_knn._C import distCUDA2
    dist2 = distCUDA2(points)          # points float32 [P, 3] on a HIP device -> float32 [P]: mean squared distance to the 3 nearest

The contract is the header's: exact float32 squared distances, self excluded by index, FLT_MAX for a missing neighbour, so P = 1 and 2
give +inf and a point with a NaN or inf coordinate gets +inf and is nobody's neighbour.  The result does not depend on the input order.
There is no CPU path: a tensor that is not on a HIP device is an error.
"""
import ctypes as C

import torch

from diff_lidargs_rasterization import _C as _base

_lib = _base._lib


def distCUDA2(points):
    """Mean squared distance of every point to its 3 nearest other points.  `points`: float32 [P, 3] on a HIP device; a view whose
    rows are evenly spaced with contiguous coordinates (e.g. xyz[:, :3] of a [P, 4] tensor) is read in place."""
    _base._require_device(points, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f"distCUDA2: `points` must have shape [P, 3], got {list(points.shape)}")
    if points.dtype != torch.float32:
        raise RuntimeError(f"distCUDA2: `points` must be float32, got {points.dtype}")
    pts = points.detach()
    P = int(pts.shape[0])
    out = torch.empty(P, dtype=torch.float32, device=pts.device)
    if P == 0:
        return out
    if pts.stride(1) != 1 or pts.stride(0) < 3:
        pts = pts.contiguous()
    nb = _lib.lidargs_knn_scratch_bytes(P)
    scratch = torch.empty(nb, dtype=torch.uint8, device=pts.device)
    with torch.cuda.device(pts.device):
        rc = _lib.lidargs_knn_mean_dist(P, C.c_void_p(pts.data_ptr()), pts.stride(0), _base._ptr(out), _base._ptr(scratch), nb,
                                        _base._stream(pts.device))
    if rc < 0:
        _base._raise(rc, "distCUDA2")
    return out
