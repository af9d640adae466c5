// selection.h -- which Gaussians a frame, a range shell or a column wedge takes: ONE definition of each test.
//
// The shell test runs twice per Gaussian on the sharded path: in the selection (shard.hip), which gathers the Gaussians of
// [lo, hi) into a rank's rows, and again in k_preprocess (preprocess.hip), which culls whatever lies outside.  The two must agree
// bit for bit, or a Gaussian on a shell boundary is rendered by two ranks or by none; so must the two forms of the selection
// (flags + scan + gather, or one launch) of either cut.  Every function here therefore rounds as written (no FMA contraction),
// whatever the including file is built with.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace lg {

// world point -> view space: A^T pw + t with A[r][k] = view[4r+k]
__device__ __forceinline__ float3 view_point(const float* vm, float3 pw) {
#pragma clang fp contract(off)
    return make_float3(vm[0] * pw.x + vm[4] * pw.y + vm[8] * pw.z + vm[12],
                       vm[1] * pw.x + vm[5] * pw.y + vm[9] * pw.z + vm[13],
                       vm[2] * pw.x + vm[6] * pw.y + vm[10] * pw.z + vm[14]);
}
__device__ __forceinline__ float range2_of(float3 p) {
#pragma clang fp contract(off)
    return p.x * p.x + p.y * p.y + p.z * p.z;
}
__device__ __forceinline__ float range_of(float3 p) { return sqrtf(range2_of(p)); }
// range shell [lo, hi) (a frame that is not a shell passes -inf, inf)
__device__ __forceinline__ bool in_shell(float dist, float lo, float hi) { return dist >= lo && dist < hi; }

// Column wedge: CAN the reference rect of a Gaussian at view-space p reach pixel columns [col_lo, col_hi)?  The exact rect needs K1;
// this is a bound from above on its half-width, from the largest scale alone:
//   every entry of the 2x2 footprint is <= A = (s_max^2 |q|^4 + 0.01) / range^2   (quaternion NOT normalised, R3/cr/forward.cu:228),
//   lambda_max <= 2 A + sqrt(1e-9) (the floor of :328-330 included), radius = sqrt(lambda), rx = ceil(3 radius / tan(2 pi / W)) (:362),
//   rect columns = [p_c - rx - 16, p_c + rx + 16) (R3/cr/auxiliary.h:80-92), + 2 pixels for atan2f rounding against K1's.
// A Gaussian taken here and found out of reach by K1 costs a preprocess row; one NOT taken can reach no pixel of the wedge.
struct WedgeSteps { float inv_col_step, inv_tan_step; };              // 1 / (2 pi / W) and 1 / tan(2 pi / W), computed on the host
inline WedgeSteps wedge_steps(int W) {
    const float pi_f = 3.14159265358979323846f;
    const float step = 2 * pi_f / (float)W;
    return {1.f / step, 1.f / tanf(step)};
}
// OPTIONAL: scales / rotations may be NULL (no scale: s_max = 0; no rotation: |q| = 1).
template <bool OPTIONAL, class I>
__device__ __forceinline__ bool wedge_reaches(float3 p, const float* scales, const float* rotations, I idx, float mod,
                                              WedgeSteps st, float col_lo, float col_hi) {
#pragma clang fp contract(off)
    const float d2 = range2_of(p);
    float smax = 0.f, nq = 1.f;
    if (!OPTIONAL || scales) smax = mod * fmaxf(fabsf(scales[3 * idx]), fmaxf(fabsf(scales[3 * idx + 1]), fabsf(scales[3 * idx + 2])));
    if (!OPTIONAL || rotations) {
        const float4 q = reinterpret_cast<const float4*>(rotations)[idx];
        nq = fmaxf(1.f, q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    }
    const float A = (smax * smax * nq * nq * 1.0001f + 0.01f) / fmaxf(d2, 1e-12f);
    const float rx = 3.f * sqrtf(2.f * A + 3.2e-5f) * st.inv_tan_step * 1.001f + 1.f;
    const float pi_f = 3.14159265358979323846f;
    const float p_c = (pi_f - atan2f(p.y, p.x)) * st.inv_col_step;
    const float reach = rx + 18.f;
    return p_c + reach >= col_lo && p_c - reach < col_hi && d2 > 0.f;
}

}  // namespace lg
