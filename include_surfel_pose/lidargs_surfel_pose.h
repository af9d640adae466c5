/*
 * lidargs_surfel_pose.h -- the gradient of the surfel rasterizer with respect to the sensor pose (no reference counterpart: the
 * reference reads viewmatrix as a constant).  DESIGN.md 4e.  The 3-D rasterizer's counterpart is include_pose/lidargs_pose.h.
 *
 * These entry points live in liblidargs_hip.so beside lidargs_surfel_backward -- they run its host sequence on the buffers of its
 * forward and share its process-wide state -- but in a header directory and under a prefix of their own (`lgsfpose_`): include/ stays
 * the drop-in boundary for the reference's interfaces, include_pose/ stays the 3-D form's three functions, and the `lidargs_*` exports of
 * the library stay exactly what include/ declares.  Conventions (device pointers, stream, return codes LIDARGS_ERR_*,
 * lidargs_last_error) are include/lidargs_rasterizer.h's; the ABI version is lidargs_abi_version()'s.
 *
 * The formula.  vm[4r + k] is element [r][k] of the transposed world->lidar matrix.  The surfel preprocess reads it in four rows, with
 * c0, c1, c2 the columns of the rotation of the normalised quaternion, m = scale_modifier, p the surfel's mean:
 *     Tu[k] = sum_r vm[4r+k] m s0 c0[r]     Tv[k] = sum_r vm[4r+k] m s1 c1[r]
 *     Tw[k] = sum_r vm[4r+k] p[r] + vm[12+k]     n[k] = sg sum_r vm[4r+k] c2[r]
 * sg = +1 where -(Tw . n) > 0 before the flip, else -1 (the normal is turned towards the sensor).  A touched surfel therefore adds, for
 * r, k < 3,
 *     dL/dvm[4r+k] += p[r] gTw[k] + m s0 c0[r] gTu[k] + m s1 c1[r] gTv[k] + sg c2[r] gn[k]        dL/dvm[12+k] += gTw[k]
 * with gTu, gTv, gn the blend's sums and gTw the final dL/dTw (the row lidargs_surfel_backward writes to dL_dtransMat[6..8], the vector
 * it rotates into dL_dmean3D).  Column 3 (elements 3, 7, 11, 15) is read by no kernel: +0.
 *   scale_modifier enters: lidargs_surfel_backward's dL_drot drops it as the reference's does, but this gradient has no reference
 *     counterpart to follow and is the true VJP of the forward's rows.  At scale_modifier = 1 the two conventions coincide.
 *   transMat_precomp is refused: precomputed rows are already in view space, their dependence on the pose is the caller's, and the
 *     caller receives dL_dtransMat from lidargs_surfel_backward.
 *   Not differentiated, as for the means: culling, the beam model's pixel decisions, the sign sg, pruning, binning and list order.
 */
#ifndef LIDARGS_SURFEL_POSE_H
#define LIDARGS_SURFEL_POSE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of view_partials for P surfels: 16 per region of 256 surfels, 0 for P <= 0. */
size_t lgsfpose_view_partial_floats(int P);

/* lidargs_surfel_backward with the gradient with respect to the sensor pose on top.  The argument list is lidargs_surfel_backward's,
 * followed by
 *   dL_dviewmatrix f32[16]: every element written (the formula above).
 *   view_partials f32[view_partial_floats]: scratch, at least lgsfpose_view_partial_floats(P) floats (64 bytes per 256 surfels), 16-byte
 *     aligned; need not be cleared, holds nothing afterwards that a caller needs.
 * Every other output is lidargs_surfel_backward's.  No float atomics in the pose sums themselves: given the same packed gradient lines
 * the 16 floats are a pure function of them (the lines are the surfel blend's float-atomic sums, which do not repeat their bits from
 * call to call).  No host read, no allocation.
 *   Refused (LIDARGS_ERR_INVALID_ARGUMENT, before any launch): what lidargs_surfel_backward refuses; dL_dviewmatrix NULL; a non-NULL
 *   transMat_precomp; for P > 0 a NULL or misaligned view_partials or view_partial_floats < lgsfpose_view_partial_floats(P).
 *   P = 0: returns 0, sixteen zeros are written. */
int lgsfpose_backward_view(
    int P, int D, int M, int R,
    const float* background,
    int width, int height,
    const float* means3D,
    const float* shs,
    const float* colors_precomp,
    const float* scales,
    float scale_modifier,
    const float* rotations,
    const float* transMat_precomp,
    const float* viewmatrix,
    const float* projmatrix,
    const float* campos,
    const float* beam_inclinations,
    const int* radii,
    char* geom_buffer,
    char* binning_buffer,
    char* image_buffer,
    const float* dL_dpix,
    const float* dL_depths,
    float* dL_dmean2D,
    float* dL_dnormal,
    float* dL_dopacity,
    float* dL_dcolor,
    float* dL_dmean3D,
    float* dL_dtransMat,
    float* dL_dtransMat_2dtemp,
    float* dL_dsh,
    float* dL_dscale,
    float* dL_drot,
    float* depth,
    int debug,
    void* stream,
    float* dL_dviewmatrix,
    float* view_partials,
    size_t view_partial_floats);

/* Test hook (never called by the binding): the chain's pose form (what lgsfpose_backward_view launches in place of the chain) and the
 * fold of its partial rows, i.e. lidargs_debug_surfel_gaussian_backward's stage 2 without transMat_precomp -- gacc as the caller filled
 * it, tlist / tcount as a stage-1 call left them, the same nine gradient arrays and depth under the same rules -- plus scale_modifier and
 * dL_dviewmatrix f32[16], view_partials and view_partial_floats as lgsfpose_backward_view's.
 *   Refused: P < 0, width <= 0, height < 2; dL_dviewmatrix NULL; for P > 0 a NULL, misaligned or short view_partials or a NULL required
 *   pointer.  P = 0: returns 0, sixteen zeros are written. */
int lgsfpose_debug_view_backward(int P, int width, int height, const float* gacc, const float* means3D, const float* scales, float scale_modifier,
                                 const float* rotations, const float* viewmatrix, const float* beams, const int* radii, float* dL_dmean2D,
                                 float* dL_dnormal, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dtransMat,
                                 float* dL_dtransMat_2dtemp, float* dL_dscale, float* dL_drot, float* depth, const unsigned char* tlist,
                                 const unsigned short* tcount, float* dL_dviewmatrix, float* view_partials, size_t view_partial_floats,
                                 void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIDARGS_SURFEL_POSE_H */
