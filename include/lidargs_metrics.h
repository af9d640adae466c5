/*
 * lidargs_metrics.h -- C ABI of the per-view evaluation of training_report (the reference's train.py:318-363): the intensity and depth
 * metrics of one rendered view, on the device, in one call.
 *
 * Inputs (device pointers, float32, row-major): render f32[2*H*W] (intensity, ray-drop), depth f32[H*W], gt f32[3*H*W] (ray-drop mask,
 * intensity, depth).  With mask = render[1] > 0.5 (strict; NaN is not > 0.5):
 *   image    = clamp(render[0], 0, 1) * mask                 (clamp keeps NaN; NaN * 0 is NaN)
 *   gt_int   = gt[1] * gt[0]
 *   e        = |image - gt_int|
 *   depth_r  = clamp(depth, depth_min, depth_max) * mask
 *   gt_depth = gt[2] * gt[0]
 *   d        = |depth_r - gt_depth|
 * out f64[11] on the device, in the order of the reference's log line (train.py:378):
 *   0 L1 = mean(e)   1 PSNR = 20 log10(1 / sqrt(mean(e*e))), float32 as torch evaluates it (+inf for a zero error)
 *   2 SSIM(image, gt_int), data_range 1: scikit-image's default algorithm (7x7 uniform window, K1 0.01, K2 0.03, sample covariance
 *     49/48, S evaluated in float32 from float32 window means, averaged in float64 over the map cropped by 3 pixels on every side)
 *   3 MAE = mean(e)   4 RMSE = sqrt(mean(e*e))   5 MedAE = lower median of e (element (n-1)/2 of the sorted values; NaN if any e is NaN)
 *   6 chamfer distance, 7 F-score: lidargs_points_meter(depth_r, gt_depth, scale 1, threshold 0.05) (include/lidargs_chamfer.h)
 *   8 depth MAE = mean(d)   9 depth MedAE = lower median of d   10 depth RMSE = sqrt(mean(d*d))
 * Every mean is a float64 sum in a fixed order, rounded to float32 after the division; sqrt / log10 are float32.  The result is
 * bit-reproducible from call to call (no float atomics).  The SSIM is restated from the published algorithm; it is not pinned against
 * scikit-image itself.  H >= 7 and W >= 7 (as scikit-image requires), H * W <= 2^28.
 * beam_inclinations f32[H] on the device (ascending) or NULL for the (fov_up, fov) intrinsics in degrees, as lidargs_points_meter.
 * scratch: lidargs_view_metrics_scratch_bytes(H, W) bytes of device memory (includes the points meter's).  The work runs on `stream`
 * with no host read, no allocation and no synchronisation, so the call can be captured in a graph.  Returns 0 or a negative
 * LIDARGS_ERR_* code (message in lidargs_last_error()).
 *
 * lidargs_view_metrics_ex: the same with with_points_meter = 0 skipping the points meter (slots 6 and 7 are then NaN).
 */
#ifndef LIDARGS_METRICS_H
#define LIDARGS_METRICS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t lidargs_view_metrics_scratch_bytes(int H, int W);

int lidargs_view_metrics(int H, int W, const float* render, const float* depth, const float* gt, float depth_min, float depth_max,
                         const float* beam_inclinations, float fov_up, float fov, double* out, char* scratch, size_t scratch_bytes,
                         void* stream);

int lidargs_view_metrics_ex(int H, int W, const float* render, const float* depth, const float* gt, float depth_min, float depth_max,
                            const float* beam_inclinations, float fov_up, float fov, int with_points_meter, double* out, char* scratch,
                            size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
