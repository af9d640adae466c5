// sweep_motion.hip -- sweep-motion compensation: the rolling-shutter warp of the means in front of an unchanged rasterizer
// (include_sweep/lidargs_sweep.h states the definition).  No reference counterpart.
//
//   k_sweep_forward<N>        one thread per Gaussian: 12 bytes in, 12 bytes out
//   k_sweep_backward<N, RED>  one thread per Gaussian, one workgroup per region of LG_REGION: recomputes the forward, reverses the N steps in
//                             registers, writes the dL_dmeans3D row; RED: the eighteen sums behind dL_dtwist and dL_dviewmatrix folded over
//                             the wave, the four waves in LDS in wave order, one 128-byte partial row per region
//   k_sweep_fold              the partial rows summed in double, in a fixed order (the idiom of k_fold_view_partials)
// No atomics: the 6 + 16 floats are a pure function of the inputs.
//
// How the lines below evaluate the definition.  With phi = t w, u = t v, m = |phi|^2 and x @ K[:3,:3] = x × w (row vectors),
//     E(t) p = p + D(p, t),   D = u + a q + b (q × phi + r) + c (r × phi),   q = p × phi,  r = u × phi,
//     a = sin(th)/th,  b = (1 - cos th)/th^2,  c = (th - sin th)/th^3,  th^2 = m           (Rodrigues and the V matrix)
// and x' = (p* - b) A^-1 = x + D(p0, t_n) A^-1: the displacement is formed and mapped back on its own, so that x' - x (metres at most)
// is not the difference of two numbers of the size of the scene, and a zero twist returns x bit for bit.  The backward is the VJP of the
// same expression, arranged the same way: with g_y = g A^-T the gradient arriving at p*, and h the gradient that reaches p0 through D and
// the iterates (everything but g_y itself),  dL/dx = g + A h,  dL/db = h,  dL/dA = x^T h - (x' - x)^T g_y  -- which is x^T (g_y + h) - x'^T g_y.
#include "lidargs_common.h"
#include "../../include/lidargs_rasterizer.h"
#include "../../include_sweep/lidargs_sweep.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int SW_ROW = 32;            // floats of a partial row: [0, 16) dL_dviewmatrix as laid out (column 3: +0), [16, 22) dL_dtwist, ten +0
constexpr float SW_SERIES_BELOW = 1.f;   // th^2 under which a, b, c and their derivatives are series (float32: the closed forms cancel there)
constexpr float SW_INV_2PI = 0.15915494309189535f, SW_PI = 3.14159265358979324f;

__device__ __forceinline__ float3 cross3(const float3 x, const float3 y) {
    return make_float3(x.y * y.z - x.z * y.y, x.z * y.x - x.x * y.z, x.x * y.y - x.y * y.x);
}
__device__ __forceinline__ float dot3f(const float3 x, const float3 y) { return x.x * y.x + x.y * y.y + x.z * y.z; }

// a, b, c of m = th^2 and (DERIV) their derivatives with respect to m
struct Coef { float a, b, c, da, db, dc; };
template <bool DERIV>
__device__ __forceinline__ Coef coef(const float m) {
    Coef k;
    if (m < SW_SERIES_BELOW) {   // seven terms: the first one left out is below 1e-11 of the value at m = 1
        k.a = 1.f + m * (-1.f / 6 + m * (1.f / 120 + m * (-1.f / 5040 + m * (1.f / 362880 + m * (-1.f / 39916800 + m * (1.f / 6227020800.f))))));
        k.b = 0.5f + m * (-1.f / 24 + m * (1.f / 720 + m * (-1.f / 40320 + m * (1.f / 3628800 + m * (-1.f / 479001600 + m * (1.f / 87178291200.f))))));
        k.c = 1.f / 6 + m * (-1.f / 120 + m * (1.f / 5040 + m * (-1.f / 362880 + m * (1.f / 39916800 + m * (-1.f / 6227020800.f + m * (1.f / 1307674368000.f))))));
        if (DERIV) {
            k.da = -1.f / 6 + m * (2.f / 120 + m * (-3.f / 5040 + m * (4.f / 362880 + m * (-5.f / 39916800 + m * (6.f / 6227020800.f)))));
            k.db = -1.f / 24 + m * (2.f / 720 + m * (-3.f / 40320 + m * (4.f / 3628800 + m * (-5.f / 479001600 + m * (6.f / 87178291200.f)))));
            k.dc = -1.f / 120 + m * (2.f / 5040 + m * (-3.f / 362880 + m * (4.f / 39916800 + m * (-5.f / 6227020800.f + m * (6.f / 1307674368000.f)))));
        }
    } else {
        const float th = sqrtf(m);
        float sn, cs;
        sincosf(th, &sn, &cs);
        k.a = sn / th; k.b = (1.f - cs) / m; k.c = (th - sn) / (m * th);
        if (DERIV) { k.da = 0.5f * (k.c - k.b); k.db = (k.a - 2.f * k.b) / (2.f * m); k.dc = (k.b - 3.f * k.c) / (2.f * m); }
    }
    return k;
}

// D(p, t): E(t) p - p
__device__ __forceinline__ float3 displace(const float3 p, const float3 w, const float3 v, const float ww, const float t) {
    const float3 phi = t * w, u = t * v;
    const Coef k = coef<false>(t * t * ww);
    const float3 q = cross3(p, phi), r = cross3(u, phi);
    return u + k.a * q + k.b * (cross3(q, phi) + r) + k.c * cross3(r, phi);
}

// s(p), and its gradient (the denominator as the header states it)
__device__ __forceinline__ float col_frac(const float3 p) { return (SW_PI - atan2f(p.y, p.x)) * SW_INV_2PI; }
__device__ __forceinline__ float3 col_frac_grad(const float3 p, const float gs) {
    const float k = gs * SW_INV_2PI / fmaxf(p.x * p.x + p.y * p.y, 1e-12f);
    return make_float3(k * p.y, -k * p.x, 0.f);
}

// The VJP of D(p, t) for the gradient g at its value: adds to gp (what reaches p through D alone), gw, gv; returns dL/dt.
__device__ __forceinline__ float displace_vjp(const float3 p, const float3 w, const float3 v, const float ww, const float t, const float3 g,
                                              float3& gp, float3& gw, float3& gv) {
    const float3 phi = t * w, u = t * v;
    const Coef k = coef<true>(t * t * ww);
    const float3 q = cross3(p, phi), r = cross3(u, phi);
    // through the three coefficients: d m / d phi = 2 phi
    const float gm = 2.f * (k.da * dot3f(g, q) + k.db * dot3f(g, cross3(q, phi) + r) + k.dc * dot3f(g, cross3(r, phi)));
    // z = x × y:  dL/dx = y × gz,  dL/dy = gz × x
    const float3 phig = cross3(phi, g);
    const float3 gq = k.a * g + k.b * phig, gr = k.b * g + k.c * phig;
    const float3 gphi = gm * phi + k.b * cross3(g, q) + k.c * cross3(g, r) + cross3(gq, p) + cross3(gr, u);
    const float3 gu = g + cross3(phi, gr);
    gp = gp + cross3(phi, gq);
    gw = gw + t * gphi;
    gv = gv + t * gu;
    return dot3f(w, gphi) + dot3f(v, gu);
}

// What every thread reads of the two small inputs (wave-uniform: scalar loads), and the inverse of A by its adjugate.
struct Pose {
    float A[3][3], Ai[3][3];
    float3 b, w, v;
    float ww;
};
__device__ __forceinline__ Pose load_pose(const float* __restrict__ vm, const float* __restrict__ xi) {
    Pose s;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) s.A[r][k] = vm[4 * r + k];
    s.b = make_float3(vm[12], vm[13], vm[14]);
    s.w = make_float3(xi[0], xi[1], xi[2]);
    s.v = make_float3(xi[3], xi[4], xi[5]);
    s.ww = dot3f(s.w, s.w);
    const float (&A)[3][3] = s.A;
    const float c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2], c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    const float id = 1.f / (A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02);
    s.Ai[0][0] = c00 * id; s.Ai[1][0] = c01 * id; s.Ai[2][0] = c02 * id;
    s.Ai[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * id; s.Ai[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) * id; s.Ai[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) * id;
    s.Ai[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * id; s.Ai[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) * id; s.Ai[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) * id;
    return s;
}
// row vector times matrix, and matrix times column vector
__device__ __forceinline__ float3 vec_mat(const float3 x, const float (&M)[3][3]) {
    return make_float3(x.x * M[0][0] + x.y * M[1][0] + x.z * M[2][0], x.x * M[0][1] + x.y * M[1][1] + x.z * M[2][1], x.x * M[0][2] + x.y * M[1][2] + x.z * M[2][2]);
}
__device__ __forceinline__ float3 mat_vec(const float (&M)[3][3], const float3 x) {
    return make_float3(M[0][0] * x.x + M[0][1] * x.y + M[0][2] * x.z, M[1][0] * x.x + M[1][1] * x.y + M[1][2] * x.z, M[2][0] * x.x + M[2][1] * x.y + M[2][2] * x.z);
}

// The times t_1 .. t_N of the iterates (tk[k - 1] = t(s_k)); every index is a compile-time constant.
template <int N>
__device__ __forceinline__ void sweep_times(const float3 p0, const Pose& s, const float t0, const float dt, float (&tk)[4]) {
    float sk = col_frac(p0);
    tk[0] = t0 + sk * dt;
#pragma unroll
    for (int k = 1; k < N; k++) {
        const float raw = col_frac(p0 + displace(p0, s.w, s.v, s.ww, tk[k - 1]));
        sk = raw + rintf(sk - raw);                                  // the seam rule: the branch of the previous iterate
        tk[k] = t0 + sk * dt;
    }
}

// One Gaussian's forward: x' - x
template <int N>
__device__ __forceinline__ float3 forward_row(const Pose& s, const float3 x, const float t0, const float dt) {
    const float3 p0 = vec_mat(x, s.A) + s.b;
    float tk[4];
    sweep_times<N>(p0, s, t0, dt, tk);
    return vec_mat(displace(p0, s.w, s.v, s.ww, tk[N - 1]), s.Ai);
}

template <int N>
__global__ void __launch_bounds__(256) k_sweep_forward(const int P, const float* __restrict__ means3D, const float* __restrict__ vm, const float* __restrict__ xi,
                                                       const float t0, const float dt, float* __restrict__ means_out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)P) return;
    const Pose s = load_pose(vm, xi);
    const float3 x = lg::get3(means3D, i);
    const float3 dx = forward_row<N>(s, x, t0, dt);
    lg::put3(means_out, i, x.x + dx.x, x.y + dx.y, x.z + dx.z);
}

// Sixteen per-lane sums folded over the wave in a fixed order (preprocess.hip k_gaussian_backward_view): halves of 32, then of 16, then
// row rotations and quad permutes.  Every lane of row L >> 4 ends with the sums of slots 4 (L >> 4) .. 4 (L >> 4) + 3.
__device__ __forceinline__ float4 wave_fold16(float (&ps)[16]) {
#pragma unroll
    for (int k = 0; k < 8; k++) ps[k] = lg::fold_halves32(ps[k], ps[k + 8]);
#pragma unroll
    for (int k = 0; k < 4; k++) ps[k] = lg::fold_halves16(ps[k], ps[k + 4]);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float x = ps[k];
        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xF, 0xF, true));   // row_ror:8
        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124, 0xF, 0xF, true));   // row_ror:4
        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
        ps[k] = x;
    }
    return make_float4(ps[0], ps[1], ps[2], ps[3]);
}

// One Gaussian's backward: returns dL/dx; pa[4r + k] and pa[12 + k] get its terms of dL/dA[r][k] and dL/db[k], px[0..5] those of dL/dxi.
template <int N>
__device__ __forceinline__ float3 backward_row(const Pose& s, const float3 x, const float3 g, const float t0, const float dt, float (&pa)[16], float (&px)[16]) {
    const float3 p0 = vec_mat(x, s.A) + s.b;
    float tk[4];
    sweep_times<N>(p0, s, t0, dt, tk);
    const float3 dx = vec_mat(displace(p0, s.w, s.v, s.ww, tk[N - 1]), s.Ai);        // x' - x
    const float3 gy = mat_vec(s.Ai, g);                                              // g A^-T: the gradient at p*
    float3 h = make_float3(0.f, 0.f, 0.f), gw = h, gv = h;
    float gs = dt * displace_vjp(p0, s.w, s.v, s.ww, tk[N - 1], gy, h, gw, gv);      // dL/ds_N
#pragma unroll
    for (int k = N - 1; k >= 1; k--) {                                               // s_{k+1} = s(E(t_k) p0) + an integer
        const float3 gq = col_frac_grad(p0 + displace(p0, s.w, s.v, s.ww, tk[k - 1]), gs);
        h = h + gq;
        gs = dt * displace_vjp(p0, s.w, s.v, s.ww, tk[k - 1], gq, h, gw, gv);
    }
    h = h + col_frac_grad(p0, gs);                                                   // s_1 = s(p0)
    const float xr[3] = {x.x, x.y, x.z}, dr[3] = {dx.x, dx.y, dx.z};
#pragma unroll
    for (int r = 0; r < 3; r++) {
        pa[4 * r + 0] = xr[r] * h.x - dr[r] * gy.x;
        pa[4 * r + 1] = xr[r] * h.y - dr[r] * gy.y;
        pa[4 * r + 2] = xr[r] * h.z - dr[r] * gy.z;
    }
    pa[12] = h.x; pa[13] = h.y; pa[14] = h.z;
    px[0] = gw.x; px[1] = gw.y; px[2] = gw.z; px[3] = gv.x; px[4] = gv.y; px[5] = gv.z;
    return g + mat_vec(s.A, h);
}

template <int N, bool RED>
__global__ void __launch_bounds__(LG_REGION) k_sweep_backward(const int P, const float* __restrict__ means3D, const float* __restrict__ vm, const float* __restrict__ xi,
                                                              const float t0, const float dt, const float* __restrict__ dL_dout, float* __restrict__ dL_dmeans3D,
                                                              float* __restrict__ partials) {
    __shared__ float4 s_part[LG_REGION / 64][SW_ROW / 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t i = (size_t)blockIdx.x * LG_REGION + tid;
    const bool live = i < (size_t)P;
    float pa[16], px[16];                                            // the lane's terms of dL_dviewmatrix and of dL_dtwist (+0 beyond P and in the unused slots)
#pragma unroll
    for (int k = 0; k < 16; k++) pa[k] = px[k] = 0.f;
    if (live) {
        const Pose s = load_pose(vm, xi);
        const float3 x = lg::get3(means3D, i), g = lg::get3(dL_dout, i);
        const float3 gx = backward_row<N>(s, x, g, t0, dt, pa, px);
        lg::put3(dL_dmeans3D, i, gx.x, gx.y, gx.z);
    }
    if (RED) {
        // (every lane of the workgroup is here: the folds are wave-wide, the barrier workgroup-wide)
        const float4 fa = wave_fold16(pa), fx = wave_fold16(px);
        if ((lane & 15) == 0) { s_part[wv][lane >> 4] = fa; s_part[wv][4 + (lane >> 4)] = fx; }
        __syncthreads();
        if (tid < SW_ROW) {
            const float* const sp = reinterpret_cast<const float*>(s_part);
            float t = sp[tid];
#pragma unroll
            for (int v = 1; v < LG_REGION / 64; v++) t += sp[v * SW_ROW + tid];          // the waves in wave order
            partials[(size_t)blockIdx.x * SW_ROW + tid] = t;
        }
    }
}

// `rows` partial rows folded in double, in a fixed order: thread (g, e) = (tid / 32, tid % 32) adds element e of rows g, g + 32, g + 64, ...
// in ascending order, thread e then adds the 32 group sums in ascending g and rounds once.  A NULL output is not written.
constexpr int SW_FOLD_GROUPS = 32;
__global__ void __launch_bounds__(SW_ROW * SW_FOLD_GROUPS) k_sweep_fold(const float* __restrict__ partials, const int rows, float* __restrict__ dL_dtwist,
                                                                        float* __restrict__ dL_dviewmatrix) {
    __shared__ double s_sum[SW_FOLD_GROUPS][SW_ROW];
    const int e = threadIdx.x & (SW_ROW - 1), g = threadIdx.x / SW_ROW;
    double acc = 0.0;
    int r = g;
    for (; r + 7 * SW_FOLD_GROUPS < rows; r += 8 * SW_FOLD_GROUPS) {   // eight loads in flight, added in row order
        float x[8];
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = partials[SW_ROW * (size_t)(r + k * SW_FOLD_GROUPS) + e];
#pragma unroll
        for (int k = 0; k < 8; k++) acc += (double)x[k];
    }
    for (; r < rows; r += SW_FOLD_GROUPS) acc += (double)partials[SW_ROW * (size_t)r + e];
    s_sum[g][e] = acc;
    __syncthreads();
    if (threadIdx.x < SW_ROW) {
        double t = 0.0;
        for (int k = 0; k < SW_FOLD_GROUPS; k++) t += s_sum[k][e];
        if (e < 16) { if (dL_dviewmatrix) dL_dviewmatrix[e] = (float)t; }
        else if (e < 22) { if (dL_dtwist) dL_dtwist[e - 16] = (float)t; }
    }
}

size_t partial_floats(int P) { return P > 0 ? SW_ROW * (((size_t)P + LG_REGION - 1) / LG_REGION) : 0; }

}  // namespace

#define SW_HIP(call) do { hipError_t e_ = (hipError_t)(call); if (e_ != hipSuccess) return lg::api_fail(LIDARGS_ERR_HIP, hipGetErrorString(e_)); } while (0)

extern "C" {

size_t lgsweep_partial_floats(int P) { return partial_floats(P); }

int lgsweep_forward(int P, const float* means3D, const float* viewmatrix, const float* twist, float t0, float t1, int iterations,
                    float* means_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "sweep_forward: P is negative");
    if (iterations < 1 || iterations > 4) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "sweep_forward: iterations must be 1..4");
    if (!isfinite(t0) || !isfinite(t1)) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "sweep_forward: the sweep times must be finite");
    if (!viewmatrix || !twist || (P > 0 && (!means3D || !means_out))) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "sweep_forward: NULL required pointer");
    if (P == 0) return 0;
    const dim3 grid((unsigned)(((size_t)P + 255) / 256)), block(256);
    const float dt = t1 - t0;
    switch (iterations) {
        case 1: hipLaunchKernelGGL(k_sweep_forward<1>, grid, block, 0, stream, P, means3D, viewmatrix, twist, t0, dt, means_out); break;
        case 2: hipLaunchKernelGGL(k_sweep_forward<2>, grid, block, 0, stream, P, means3D, viewmatrix, twist, t0, dt, means_out); break;
        case 3: hipLaunchKernelGGL(k_sweep_forward<3>, grid, block, 0, stream, P, means3D, viewmatrix, twist, t0, dt, means_out); break;
        default: hipLaunchKernelGGL(k_sweep_forward<4>, grid, block, 0, stream, P, means3D, viewmatrix, twist, t0, dt, means_out); break;
    }
    return lg::api_check_launch(stream, 0, "sweep_forward");
}

int lgsweep_backward(int P, const float* means3D, const float* viewmatrix, const float* twist, float t0, float t1, int iterations,
                     const float* dL_dmeans_out, float* dL_dmeans3D, float* dL_dtwist, float* dL_dviewmatrix, float* partials,
                     size_t partial_floats_given, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "sweep_backward: P is negative");
    if (iterations < 1 || iterations > 4) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "sweep_backward: iterations must be 1..4");
    if (!isfinite(t0) || !isfinite(t1)) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "sweep_backward: the sweep times must be finite");
    if (!viewmatrix || !twist || (P > 0 && (!means3D || !dL_dmeans_out || !dL_dmeans3D)))
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "sweep_backward: NULL required pointer");
    const bool reduce = dL_dtwist || dL_dviewmatrix;
    if (P > 0 && reduce && (!partials || ((uintptr_t)partials & 15u) || partial_floats_given < partial_floats(P)))
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "sweep_backward: partials is NULL, not 16-byte aligned or shorter than lgsweep_partial_floats(P)");
    if (P == 0) {
        if (dL_dtwist) SW_HIP(hipMemsetAsync(dL_dtwist, 0, 6 * sizeof(float), stream));
        if (dL_dviewmatrix) SW_HIP(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float), stream));
        return 0;
    }
    const unsigned regions = (unsigned)(((size_t)P + LG_REGION - 1) / LG_REGION);
    const dim3 grid(regions), block(LG_REGION);
    const float dt = t1 - t0;
#define SW_LAUNCH(N)                                                                                                                                       \
    if (reduce) hipLaunchKernelGGL((k_sweep_backward<N, true>), grid, block, 0, stream, P, means3D, viewmatrix, twist, t0, dt, dL_dmeans_out, dL_dmeans3D, partials); \
    else hipLaunchKernelGGL((k_sweep_backward<N, false>), grid, block, 0, stream, P, means3D, viewmatrix, twist, t0, dt, dL_dmeans_out, dL_dmeans3D, partials)
    switch (iterations) {
        case 1: SW_LAUNCH(1); break;
        case 2: SW_LAUNCH(2); break;
        case 3: SW_LAUNCH(3); break;
        default: SW_LAUNCH(4); break;
    }
#undef SW_LAUNCH
    if (reduce) hipLaunchKernelGGL(k_sweep_fold, dim3(1), dim3(SW_ROW * SW_FOLD_GROUPS), 0, stream, partials, (int)regions, dL_dtwist, dL_dviewmatrix);
    return lg::api_check_launch(stream, 0, "sweep_backward");
}

}  // extern "C"
