"""A numpy restatement of the per-view metric contract of include/lidargs_metrics.h (the reference's train.py:318-363), the yardstick of
tests/test_view_metrics_*.py.

SSIM: scikit-image's default algorithm (structural_similarity, scikit-image >= 0.19, float32 inputs) restated from its publication --
7 x 7 uniform window, K1 0.01, K2 0.03, sample covariance 49/48, S in float32 from float32 window means, the float64 mean of the map
cropped by 3 pixels.  The window sums are float64 box sums through cumulative sums (no scipy).  Not pinned against scikit-image itself,
which is not available where these tests run.
Medians: np.partition at (n - 1) // 2 (torch.median's lower median), NaN when any value is NaN."""
import numpy as np

NAMES = ("l1", "psnr", "ssim", "in_mae", "in_rmse", "in_medae", "cd", "fscore", "mae", "medae", "rmse")


def prepare(render, depth, gt, depth_min, depth_max):
    """-> image, gt_int, depth_r, gt_depth (float32 [H, W]) as train.py:318-363 computes them."""
    render, depth, gt = (np.asarray(a, np.float32) for a in (render, depth, gt))
    with np.errstate(invalid="ignore"):
        mask = (render[1] > np.float32(0.5)).astype(np.float32)
        c = render[0]
        img = np.where(np.isnan(c), c, np.minimum(np.maximum(c, np.float32(0)), np.float32(1))) * mask
        dv = depth[0]
        dr = np.where(np.isnan(dv), dv, np.minimum(np.maximum(dv, np.float32(depth_min)), np.float32(depth_max))) * mask
    return img.astype(np.float32), (gt[1] * gt[0]).astype(np.float32), dr.astype(np.float32), (gt[2] * gt[0]).astype(np.float32)


def _box7(a):
    """float64 7 x 7 window sums of the in-bounds windows: [H - 6, W - 6]."""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1))
    c[1:, 1:] = np.cumsum(np.cumsum(a.astype(np.float64), 0), 1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def ssim(x, y):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    if x.shape[0] < 7 or x.shape[1] < 7:
        raise ValueError("ssim: the 7 x 7 window needs H >= 7 and W >= 7")
    m = lambda a: (_box7(a) / 49.0).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ux, uy, uxx, uyy, uxy = m(x), m(y), m(x * x), m(y * y), m(x * y)
        cov_norm = np.float32(49.0 / 48.0)
        C1, C2 = np.float32(0.01 * 0.01), np.float32(0.03 * 0.03)
        vx = cov_norm * (uxx - ux * ux)
        vy = cov_norm * (uyy - uy * uy)
        vxy = cov_norm * (uxy - ux * uy)
        A1, A2 = np.float32(2) * ux * uy + C1, np.float32(2) * vxy + C2
        B1, B2 = ux * ux + uy * uy + C1, vx + vy + C2
        S = (A1 * A2) / (B1 * B2)
    assert S.dtype == np.float32
    return float(S.mean(dtype=np.float64))


def lower_median(a):
    a = np.asarray(a, np.float32).ravel()
    if np.isnan(a).any():
        return float("nan")
    k = (a.size - 1) // 2
    return float(np.partition(a, k)[k])


def _mean32(a):
    return float(np.float32(np.asarray(a, np.float32).astype(np.float64).sum() / a.size))


def view_metrics(render, depth, gt, depth_min=5.0, depth_max=80.0, points=None):
    """-> float64[11] in NAMES order.  points: a callable (depth_r, gt_depth) -> (chamfer, F-score), or None for NaN in slots 6, 7."""
    img, gti, dr, gd = prepare(render, depth, gt, depth_min, depth_max)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e = np.abs(img - gti)
        d = np.abs(dr - gd)
        mse = np.float32(_mean32(e * e))
        psnr = np.float32(20) * np.log10(np.float32(1) / np.sqrt(mse))
        msd = np.float32(_mean32(d * d))
    cd, fs = points(dr, gd) if points is not None else (float("nan"), float("nan"))
    return np.array([_mean32(e), float(psnr), ssim(img, gti), _mean32(e), float(np.sqrt(mse)), lower_median(e), cd, fs,
                     _mean32(d), lower_median(d), float(np.sqrt(msd))], np.float64)
