/*
 * lidargs_pose.h -- the gradient of the 3-D rasterizer with respect to the sensor pose (no reference counterpart: the reference reads
 * viewmatrix as a constant).  DESIGN.md 4e.
 *
 * These entry points live in liblidargs_hip.so beside lidargs_backward -- they run its host sequence on the buffers of its forward and
 * share its process-wide state -- but in a header directory and under a prefix of their own (`lgpose_`): include/ stays the drop-in
 * boundary for the reference's interfaces, and the `lidargs_*` exports of the library stay exactly what include/ declares.  Conventions
 * (device pointers, stream, return codes LIDARGS_ERR_*, lidargs_last_error) are include/lidargs_rasterizer.h's; the ABI version is
 * lidargs_abi_version()'s.
 */
#ifndef LIDARGS_POSE_H
#define LIDARGS_POSE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* lidargs_backward with the gradient with respect to the sensor pose on top.  The argument list is lidargs_backward's, followed by
 *   dL_dviewmatrix f32[16]: every element written.  Element 4r + k is dL/d viewmatrix[r][k] of the transposed world->lidar matrix as
 *     the kernels read it: the view-space mean pv[k] = sum_r vm[4r+k] p[r] + vm[12+k] and the world-space tangents t_i[r] = sum_k
 *     vm[4r+k] u_i[k].  Column 3 (elements 3, 7, 11, 15) is read by no kernel: +0.  The formulas are the reference backward's as written
 *     (damped conic included), not a re-derived analytic gradient; culling, the beam bisection, binning and list order are not
 *     differentiated, as for the means.
 *   view_partials f32[view_partial_floats]: scratch, at least lgpose_view_partial_floats(P) floats (64 bytes per 256 Gaussians), 16-byte
 *     aligned; need not be cleared, holds nothing afterwards that a caller needs.
 * Every other output is lidargs_backward's, bit for bit.  No float atomics on this path: given the same packed gradient lines the 16
 * floats are a pure function of them (with LIDARGS_DETERMINISTIC=1 buffers: of the call's inputs).  Works on default, deterministic,
 * median and strongest buffers of lidargs_forward / lidargs_forward_enqueue; no host read, no allocation, graph-capturable.
 *   Refused (LIDARGS_ERR_INVALID_ARGUMENT, before any launch): what lidargs_backward refuses; dL_dviewmatrix NULL; for P > 0 a NULL or
 *   misaligned view_partials or view_partial_floats < lgpose_view_partial_floats(P).  P = 0: returns 0, sixteen zeros are written.
 * Shell and wedge buffers have no such entry point: no gradient reaches their view matrix.  Surfel buffers: include_surfel_pose/lidargs_surfel_pose.h. */
size_t lgpose_view_partial_floats(int P);
int lgpose_backward_view(
    int P, int D, int M, int R,
    const float* background,
    int width, int height,
    const float* means3D,
    const float* shs,
    const float* colors_precomp,
    const float* scales,
    float scale_modifier,
    const float* rotations,
    const float* cov3D_precomp,
    const float* viewmatrix,
    const float* projmatrix,
    const float* campos,
    const float* beam_inclinations,
    float tan_fovx, float tan_fovy,
    const int* radii,
    char* geom_buffer,
    char* binning_buffer,
    char* image_buffer,
    const float* dL_dpix,
    const float* dL_dout_depth,
    const float* dL_dout_occ,
    float* dL_dmean2D,
    float* dL_dconic,
    float* dL_dopacity,
    float* dL_dcolor,
    float* dL_ddepths,
    float* dL_dmean3D,
    float* dL_dsphere_means3D,
    float* dL_dbasis_u1,
    float* dL_dbasis_u2,
    float* dL_dcov3D,
    float* dL_dsh,
    float* dL_dscale,
    float* dL_drot,
    int debug,
    void* stream,
    float* dL_dviewmatrix,
    float* view_partials,
    size_t view_partial_floats);

/* Test hook (never called by the binding): the chain's pose form (what lgpose_backward_view launches in place of the chain) and the
 * fold of its partial rows, i.e. lidargs_debug_gaussian_backward's stage 2 -- gacc as the caller filled it, tlist / tcount as a stage-1
 * call left them, the same twelve gradient arrays under the same rules -- plus dL_dviewmatrix f32[16], view_partials and
 * view_partial_floats as lgpose_backward_view's.  mode_word / acc64 (both or neither; NULL: plain float lines): a device word and
 * i64[16 P]; where the word has bit 0 set the lines are read as a deterministic forward's buffers hold them -- gacc carries each slot's
 * largest term, acc64 the fixed-point sums on the grid that term fixes (csrc/lidargs_common.h "deterministic accumulation").
 *   Refused: P < 0; dL_dviewmatrix NULL; for P > 0 a NULL, misaligned or short view_partials, a NULL required pointer, one of mode_word /
 *   acc64 without the other.  P = 0: returns 0, sixteen zeros are written. */
int lgpose_debug_view_backward(int P, const float* gacc, const float* means3D, const float* scales, float scale_modifier, const float* rotations,
                               const float* cov3D_precomp, const float* viewmatrix, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                               float* dL_dcolor, float* dL_ddepths, float* dL_dmean3D, float* dL_dsphere_means3D, float* dL_dbasis_u1,
                               float* dL_dbasis_u2, float* dL_dcov3D, float* dL_dscale, float* dL_drot, const unsigned char* tlist,
                               const unsigned short* tcount, const unsigned* mode_word, const long long* acc64, float* dL_dviewmatrix,
                               float* view_partials, size_t view_partial_floats, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIDARGS_POSE_H */
