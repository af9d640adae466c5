/*
 * lidargs_sweep.h -- sweep-motion compensation: a rolling-shutter warp of the means in front of an unchanged rasterizer (no reference
 * counterpart: the reference renders a sweep as if every column had been measured at one instant).  DESIGN.md 4f.
 *
 * Definition (stated here once; everything else cites it).
 *   vm    viewmatrix f32[16] as the kernels read it: p0[k] = sum_r x[r] vm[4r + k] + vm[12 + k].  A = vm[:3,:3], b = vm[3,:3]; A may be
 *         any invertible matrix.
 *   xi    twist f32[6] = (w, v): rotation vector, then translation, the se(3) chart of INTEGRATION.md 3, row-vector convention:
 *         T(xi) = matrix_exp(K), K[2][1] = w0, K[0][2] = w1, K[1][0] = w2, K[1][2] = -w0, K[2][0] = -w1, K[0][1] = -w2, K[3][:3] = v.  The
 *         sensor pose at time t is vm @ T(t xi); hence E(t) p = ([p, 1] @ T(t xi))[:3].
 *   s(p)  = (pi - atan2(p.y, p.x)) / (2 pi): the fraction of the image width, the column convention of both preprocess kernels.
 *   t(s)  = t0 + s (t1 - t0).  (t0, t1) = (-0.5, 0.5): vm is the mid-sweep pose and xi the motion per sweep; a sensor whose columns run
 *         against time swaps the two.
 *   Iterates, n = iterations in 1..4:  s_1 = s(p0);  for k = 2..n:  raw = s(E(t(s_{k-1})) p0),  s_k = raw + round(s_{k-1} - raw).  The last
 *         step is the seam rule: later iterates stay on the branch of the previous one, so s_k may leave [0, 1).  round carries no gradient.
 *   Output  p* = E(t(s_n)) p0,  x' = (p* - b) A^-1: the world-space mean to hand the rasterizer.
 *   Backward  the exact VJP of this n-step expression with respect to x, xi and vm.  atan2's derivative uses the denominator
 *         max(p.x^2 + p.y^2, 1e-12).  Through the inverse dL/dA gets -x'^T g_y per Gaussian, g_y = g A^-T, g the gradient arriving at x'.
 *         Column 3 of dL/dvm is +0, as in lidargs_pose.h.  With xi = 0 the op is the identity and dL/dvm is zero.
 *   Limits  covariances are not rotated (the neglected angle is at most |w| max(|t0|, |t1|)); a footprint takes one time, that of its
 *         centre; the iteration contracts only while |v| |t1 - t0| << 2 pi rho (near the sensor's axis it does not); a point within motion
 *         reach of the seam is, physically, seen twice or never, and the seam rule picks the continuous branch.
 *
 * These entry points live in liblidargs_hip.so under a prefix and in a header directory of their own (`lgsweep_`), as include_pose/ does:
 * include/ stays the drop-in boundary for the reference's interfaces.  Conventions (device pointers, stream, return codes LIDARGS_ERR_*,
 * lidargs_last_error) are include/lidargs_rasterizer.h's; the ABI version is lidargs_abi_version()'s.  Neither function reads anything
 * back to the host or allocates: both are graph-capturable.  No float atomics: the outputs are a pure function of the inputs.
 */
#ifndef LIDARGS_SWEEP_H
#define LIDARGS_SWEEP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of `partials` for P Gaussians: 32 per region of 256 Gaussians (0 for P <= 0). */
size_t lgsweep_partial_floats(int P);

/* means_out f32[3P] = x' of means3D f32[3P] (24 bytes per Gaussian).  viewmatrix f32[16] and twist f32[6] are DEVICE memory.
 *   Refused (LIDARGS_ERR_INVALID_ARGUMENT, before any launch): P < 0; a NULL viewmatrix or twist; for P > 0 a NULL means3D or means_out;
 *   iterations outside 1..4; a non-finite t0 or t1.  P = 0: returns 0. */
int lgsweep_forward(int P, const float* means3D, const float* viewmatrix, const float* twist, float t0, float t1, int iterations,
                    float* means_out, void* stream);

/* The VJP for dL_dmeans_out f32[3P], the gradient arriving at x'.  Recomputes the forward from the inputs (nothing else is saved).
 *   dL_dmeans3D f32[3P]: every row written.
 *   dL_dtwist f32[6] or NULL, dL_dviewmatrix f32[16] or NULL (element 4r + k is dL/d viewmatrix[r][k]; elements 3, 7, 11, 15 are +0):
 *     written in full where given, through
 *   partials f32[partial_floats]: scratch, at least lgsweep_partial_floats(P) floats, 16-byte aligned; need not be cleared, holds nothing
 *     afterwards that a caller needs; not touched when both reduced gradients are NULL.
 *   Refused (LIDARGS_ERR_INVALID_ARGUMENT, before any launch): what lgsweep_forward refuses (dL_dmeans_out and dL_dmeans3D in the place of
 *   means_out); for P > 0 and a reduced gradient asked for, a NULL or misaligned partials or partial_floats < lgsweep_partial_floats(P).
 *   P = 0: returns 0, the reduced gradients that were asked for are written as zeros. */
int lgsweep_backward(int P, const float* means3D, const float* viewmatrix, const float* twist, float t0, float t1, int iterations,
                     const float* dL_dmeans_out, float* dL_dmeans3D, float* dL_dtwist, float* dL_dviewmatrix, float* partials,
                     size_t partial_floats, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIDARGS_SWEEP_H */
