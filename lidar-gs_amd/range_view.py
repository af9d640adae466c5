"""`range_view` -- the reference's range-view conversion (utils/lidar_utils.py:51-110, :171-232, :296-299) on the device.

    from range_view import lidar_to_pano_with_intensities, pano_to_lidar, pano_to_lidar_with_intensities, get_beam_inclinations

Same names, same arguments (without `cam_pos`, which the reference cannot take either: its `cam_pos != None` fails on arrays).  Device
tensors in give float32 device tensors out; numpy arrays in give numpy float64 out, as the reference returns, through one upload and one
read.  Two keyword arguments are new: `transform`, a 3x4 or 4x4 [R | t] applied to the points in double inside the kernel (world -> sensor
for the projection, sensor -> world for the back-projection: `np.pad(...) @ l2w.T` of scene/dataset_readers.py:433), and `pixel_rows`,
which makes the projection put a ray into the pixel `pano_to_lidar` and the rasterizer give it (the reference's own projection writes one
row lower and drops azimuth -pi; include_rangeview/lidargs_range_view.h).  `ray_dirs` is the [H, W, 3] table of
scene/dataset_readers.py:446-455.

Where the projection deliberately differs from the reference: points of range 0 and points with a NaN or inf are dropped (the reference
leaves the intensity of a zero-range point in an otherwise empty pixel, and raises on a NaN).

`N == 0` and an all-empty numpy image are answered without a native call.  An all-empty DEVICE image is not looked at on the host first (that
would be a read of its own): it goes through the native call like any other and comes back as `[0, 4]` after the one read of the count.

There is NO numpy path: what the native library cannot take is a RuntimeError or ValueError, never a fallback.
"""
import ctypes as C

import numpy as np
import torch

import lidargs_abi
from lidargs_abi import ptr as _ptr, stream as _stream

_lib = lidargs_abi.library("rangeview")
ABI_VERSION, PIXEL_ROWS = (lidargs_abi.library_constants("rangeview")["LIDARGS_RV_" + k] for k in ("ABI_VERSION", "PIXEL_ROWS"))


def get_beam_inclinations(fov_up, fov, H):
    """utils/lidar_utils.py:296-299: the ascending float32 table of a uniform (fov_up, fov) sensor, on the host."""
    j = np.arange(H, dtype=np.float32)
    return ((fov_up - j / H * fov) / 180 * np.pi)[::-1]


def _check(rc, what):
    lidargs_abi.check(_lib, rc, "range_view." + what)


def _image(x, name, what):
    """(x, came_from_numpy): a device tensor is checked (float32) and made contiguous; a numpy array is passed on for its one upload."""
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError(f"range_view.{what}: `{name}` is a CPU tensor; pass a tensor on a HIP device (device='cuda') or a numpy array. "
                               "There is no CPU path and no fallback to one")
        if x.dtype != torch.float32:
            raise RuntimeError(f"range_view.{what}: `{name}` must be float32, got {x.dtype}")
        return x.detach().contiguous(), False
    if isinstance(x, np.ndarray):
        if x.dtype.kind != "f":
            raise RuntimeError(f"range_view.{what}: `{name}` must be a floating-point array, got {x.dtype}")
        return x, True
    raise RuntimeError(f"range_view.{what}: `{name}` must be a device tensor or a numpy array, got {type(x).__name__}")


def _rows(H, lidar_K, beam_inclinations, what):
    """(host float32 beam table or None, fov_up, fov), checked."""
    if (lidar_K is None) == (beam_inclinations is None):
        raise ValueError(f"range_view.{what}: give exactly one of `lidar_K` = (fov_up, fov) and `beam_inclinations`")
    if beam_inclinations is None:
        fov_up, fov = float(lidar_K[0]), float(lidar_K[1])
        if not fov > 0.0:
            raise ValueError(f"range_view.{what}: lidar_K = (fov_up, fov) needs fov > 0, got {fov}")
        return None, fov_up, fov
    b = beam_inclinations.detach().cpu().numpy() if isinstance(beam_inclinations, torch.Tensor) else np.asarray(beam_inclinations)
    if b.ndim != 1 or b.shape[0] != H or b.dtype.kind not in "fiu":
        raise ValueError(f"range_view.{what}: `beam_inclinations` must be {H} numbers, one per image row, got shape {list(b.shape)} {b.dtype}")
    b = np.ascontiguousarray(b, dtype=np.float32)            # evaluated in float32 (a float64 table is rounded first)
    if not np.all(np.isfinite(b)) or np.any(np.diff(b) < 0):
        raise ValueError(f"range_view.{what}: `beam_inclinations` must be finite and ascending")
    return b, 0.0, 0.0


def _transform(transform, what):
    """None or a ctypes array of the 12 doubles of a 3x4 [R | t] (the last row of a 4x4 must be 0 0 0 1)."""
    if transform is None:
        return None
    m = transform.detach().cpu().numpy() if isinstance(transform, torch.Tensor) else np.asarray(transform)
    m = np.asarray(m, dtype=np.float64)
    if m.shape == (4, 4) and np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
        m = m[:3]
    if m.shape != (3, 4) or not np.all(np.isfinite(m)):
        raise ValueError(f"range_view.{what}: `transform` must be a finite 3x4, or a 4x4 with last row (0, 0, 0, 1), got shape {list(m.shape)}")
    return (C.c_double * 12)(*m.reshape(-1).tolist())


def _device(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("range_view: no HIP device (torch.cuda.is_available() is False); there is no CPU path and no fallback to one")
    return torch.device("cuda", torch.cuda.current_device())


def _beams_on(beams, beam_inclinations, dev):
    if beams is None:
        return None
    if isinstance(beam_inclinations, torch.Tensor) and beam_inclinations.is_cuda and beam_inclinations.dtype == torch.float32 \
            and beam_inclinations.device == dev:
        return beam_inclinations.detach().contiguous()
    return torch.from_numpy(beams).to(dev)


def lidar_to_pano_with_intensities(local_points_with_intensities, lidar_H, lidar_W, lidar_K=None, beam_inclinations=None, max_depth=80, *,
                                   transform=None, pixel_rows=False):
    """utils/lidar_utils.py:51-110.  points [N, 4] (x, y, z, intensity) -> (pano [H, W], intensities [H, W]): per pixel the smallest range
    below `max_depth` and its intensity, (0, 0) where no point fell; among equal ranges the first point in input order."""
    what = "lidar_to_pano_with_intensities"
    H, W = int(lidar_H), int(lidar_W)
    if H <= 0 or W <= 0 or H * W > 1 << 28:
        raise ValueError(f"range_view.{what}: bad image size {H} x {W}")
    pts, from_numpy = _image(local_points_with_intensities, "points", what)
    if pts.ndim != 2 or pts.shape[1] != 4:
        raise RuntimeError(f"range_view.{what}: `points` must be [N, 4] (x, y, z, intensity), got {list(pts.shape)}")
    N = int(pts.shape[0])
    if N >= 1 << 31:
        raise ValueError(f"range_view.{what}: {N} points; the pixel keys hold the point's index in 32 bits and the C ABI takes N as int (N < 2^31)")
    if isinstance(beam_inclinations, torch.Tensor) and beam_inclinations.is_cuda and from_numpy:
        raise RuntimeError(f"range_view.{what}: numpy points with a device beam table: pass all on the host or all on the device")
    beams, fov_up, fov = _rows(H, lidar_K, beam_inclinations, what)
    xf = _transform(transform, what)
    if N == 0:
        if from_numpy:
            return np.zeros((H, W)), np.zeros((H, W))
        return torch.zeros(H, W, dtype=torch.float32, device=pts.device), torch.zeros(H, W, dtype=torch.float32, device=pts.device)
    dev = _device(pts)
    if from_numpy:
        pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(dev)
    out = torch.empty(2, H, W, dtype=torch.float32, device=dev)
    nb = _lib.lidargs_rv_scratch_bytes(H, W)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    bt = _beams_on(beams, beam_inclinations, dev)
    with torch.cuda.device(dev):
        _check(_lib.lidargs_rv_project(N, _ptr(pts), H, W, _ptr(bt), fov_up, fov, float(max_depth), xf, PIXEL_ROWS if pixel_rows else 0,
                                       _ptr(out[0]), _ptr(out[1]), _ptr(scratch), nb, _stream(dev)), what)
    if from_numpy:
        host = out.cpu().numpy().astype(np.float64)          # one read
        return host[0], host[1]
    return out[0], out[1]


def pano_to_lidar_with_intensities(pano, intensities, lidar_K=None, beam_inclinations=None, *, transform=None):
    """utils/lidar_utils.py:171-214.  (pano [H, W], intensities [H, W] or None) -> [n, 4]: a point (x, y, z, intensity) of every pixel with
    pano != 0, in row-major pixel order."""
    what = "pano_to_lidar_with_intensities"
    pano, from_numpy = _image(pano, "pano", what)
    if pano.ndim != 2 or pano.shape[0] == 0 or pano.shape[1] == 0:
        raise RuntimeError(f"range_view.{what}: `pano` must be a non-empty [H, W] image, got {list(pano.shape)}")
    H, W = int(pano.shape[0]), int(pano.shape[1])
    if H * W > 1 << 28:
        raise ValueError(f"range_view.{what}: bad image size {H} x {W}")
    inten = None
    if intensities is not None:
        inten, inten_numpy = _image(intensities, "intensities", what)
        if inten_numpy != from_numpy:
            raise RuntimeError(f"range_view.{what}: `pano` and `intensities` must both be device tensors or both numpy arrays")
        if int(np.prod(inten.shape)) != H * W:
            raise RuntimeError(f"range_view.{what}: `intensities` must have the pano's {H} x {W} elements, got {list(inten.shape)}")
        if not from_numpy and inten.device != pano.device:
            raise RuntimeError(f"range_view.{what}: `pano` and `intensities` are on different devices")
    if isinstance(beam_inclinations, torch.Tensor) and beam_inclinations.is_cuda and from_numpy:
        raise RuntimeError(f"range_view.{what}: a numpy pano with a device beam table: pass all on the host or all on the device")
    beams, fov_up, fov = _rows(H, lidar_K, beam_inclinations, what)
    xf = _transform(transform, what)
    if from_numpy:
        if not np.any(pano != 0):
            return np.zeros((0, 4))
        dev = _device()
        both = np.stack([pano, np.zeros_like(pano) if inten is None else inten.reshape(H, W)]).astype(np.float32)
        both = torch.from_numpy(both).to(dev)                # one upload
        pano, inten = both[0], both[1]
    dev = pano.device
    out = torch.empty(H * W, 4, dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)    # (the library's u32; at most H * W <= 2^28)
    nb = _lib.lidargs_rv_scratch_bytes(H, W)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    bt = _beams_on(beams, beam_inclinations, dev)
    with torch.cuda.device(dev):
        _check(_lib.lidargs_rv_unproject(H, W, _ptr(pano), _ptr(inten), _ptr(bt), fov_up, fov, xf, _ptr(out), _ptr(count), _ptr(scratch), nb,
                                         _stream(dev)), what)
    n = int(count.item())                                    # the one read of the count
    if from_numpy:
        return out[:n].cpu().numpy().astype(np.float64)
    return out[:n].clone() if n < H * W else out             # exact size: the capacity is not kept alive behind a view


def pano_to_lidar(pano, lidar_K=None, beam_inclinations=None, *, transform=None):
    """utils/lidar_utils.py:216-232: the [n, 3] points of the non-empty pixels."""
    p = pano_to_lidar_with_intensities(pano, None, lidar_K=lidar_K, beam_inclinations=beam_inclinations, transform=transform)
    return np.ascontiguousarray(p[:, :3]) if isinstance(p, np.ndarray) else p[:, :3].contiguous()


def ray_dirs(H, W, lidar_K=None, beam_inclinations=None, device=None):
    """scene/dataset_readers.py:446-455: the unit ray of every pixel, float32 [H, W, 3] on the device."""
    what = "ray_dirs"
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H * W > 1 << 28:
        raise ValueError(f"range_view.{what}: bad image size {H} x {W}")
    beams, fov_up, fov = _rows(H, lidar_K, beam_inclinations, what)
    dev = torch.device(device) if device is not None else _device(beam_inclinations)
    out = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    bt = _beams_on(beams, beam_inclinations, dev)
    with torch.cuda.device(dev):
        _check(_lib.lidargs_rv_ray_dirs(H, W, _ptr(bt), fov_up, fov, _ptr(out), _stream(dev)), what)
    return out
