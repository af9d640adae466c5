/*
 * lidargs_range_view.h -- C ABI of the range-view conversion (liblidargs_rangeview.so, built from csrc/range_view.hip alone).
 *
 * The two directions between a point cloud and a range image, on the device:
 *   lidargs_rv_project     lidar_to_pano_with_intensities   (utils/lidar_utils.py:51-110): points -> (pano, intensity), minimum range per pixel
 *   lidargs_rv_unproject   pano_to_lidar_with_intensities   (utils/lidar_utils.py:171-214): the non-empty pixels -> points, row-major order
 *   lidargs_rv_ray_dirs    the per-pixel unit rays          (scene/dataset_readers.py:446-455)
 *
 * Every array pointer is a DEVICE pointer; `world_to_sensor` / `sensor_to_world` are HOST pointers to 12 doubles (a 3x4 row-major
 * [R | t], applied in double as ((r0*x + r1*y) + r2*z) + t and rounded once to float32) or NULL for none.  `beams` is the table of
 * beam inclinations in radians, f32[H], ascending (not checked here), or NULL: then (fov_up, fov) in degrees give the rows.
 * `points` and `out_points` are rows of four floats and must be 16-byte aligned.
 * `scratch` holds lidargs_rv_scratch_bytes(H, W) bytes, 8-byte aligned; nothing is assumed about its content and nothing is kept in it.
 *
 * project -- all arithmetic in float32, each operation rounded as written (the library is built without contraction):
 *   dist = sqrtf((x*x + y*y) + z*z);                       dropped: dist >= max_depth, dist == 0, any of x y z intensity dist not finite
 *   c    = rintf((pi_f - atan2f(y, x)) / (float)(2 pi / W))                                           (ties to even)
 *   beams:  a = atan2f(z, sqrtf(x*x + y*y));  label = nearest beam (the lower one on a tie, clamped at both ends);  r = H - label
 *   fov:    a = atan2f(z, sqrtf(x*x + y*y)) + (float)((fov - fov_up) / 180 pi);  r = rintf(H - a / (float)(fov / 180 pi / H))
 *   dropped: r or c outside the image.  The pixel keeps the smallest dist; among equal dists the point of the lowest index.
 *   flags = 0: the reference's convention as above (with a beam table row 0 is never written; column W is dropped).
 *   flags = LIDARGS_RV_PIXEL_ROWS: r = H - 1 - label and column W wraps to 0 -- the pixel the rasterizer and lidargs_rv_unproject
 *   give that ray.  (In fov mode the rows already agree; only the column wrap changes.)
 *   Every pixel of out_pano and out_intensity is written: (0, 0) where no point fell.
 *
 * unproject -- point of pixel (row j, column i) with pano != 0:
 *   beta = -(i - W/2) / W * 2 * pi_f;  alpha = beams[H-1-j]  or  (fov_up - j / H * fov) / 180 * pi_f          (float32)
 *   (cos alpha cos beta, cos alpha sin beta, sin alpha) * pano, cos / sin correctly rounded; column 3 = intensity (0 when NULL).
 *   out_points f32[H*W*4] is the capacity; the first *out_count rows are written, in row-major pixel order.
 *
 * Each function returns 0, or a negative code with a message in lidargs_rv_last_error() (thread-local): -1 an invalid argument
 * (sizes, NULL pointer, fov <= 0 without a beam table, scratch too small), -4 a HIP error.  Arguments are validated before any
 * device work.  N == 0 is valid (an empty image).  H * W is at most 2^28.
 */
#ifndef LIDARGS_RANGE_VIEW_H
#define LIDARGS_RANGE_VIEW_H

#include <stddef.h>

#define LIDARGS_RV_ABI_VERSION 1
#define LIDARGS_RV_PIXEL_ROWS 1

#ifdef __cplusplus
extern "C" {
#endif

size_t lidargs_rv_scratch_bytes(int H, int W);
int lidargs_rv_project(int N, const float* points, int H, int W, const float* beams, float fov_up, float fov, float max_depth,
                       const double* world_to_sensor, int flags, float* out_pano, float* out_intensity,
                       char* scratch, size_t scratch_bytes, void* stream);
int lidargs_rv_unproject(int H, int W, const float* pano, const float* intensity, const float* beams, float fov_up, float fov,
                         const double* sensor_to_world, float* out_points, unsigned* out_count, char* scratch, size_t scratch_bytes, void* stream);
int lidargs_rv_ray_dirs(int H, int W, const float* beams, float fov_up, float fov, float* out_dirs, void* stream);
const char* lidargs_rv_last_error(void);
int lidargs_rv_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
