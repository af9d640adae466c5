// preprocess.hip -- per-Gaussian streaming kernels (gfx950).
//
//   k_setup_tables      per-row / per-column ray tables
//   k_preprocess        K1 (R3/cr/forward.cu:256-384) and, with FILTER, K2 (:388-497)
//   k_mark_visible      K11 (R3/cr/rasterizer_impl.cu:54-66)
//   k_gaussian_backward K9 + K10 fused (R3/cr/backward.cu:157-382, :453-532, :385-448)
//   k_gaussian_backward_view / k_fold_view_partials   the same chain + the gradient with respect to the view matrix (no reference counterpart)
//   k_zero_touched / k_touch_visible   the touched-Gaussian lists the backward starts from
//
// All of them are one-thread-per-Gaussian HBM streams: 44 B in, <= 100 B out per Gaussian for
// preprocess.  The arithmetic is a re-derivation (vector form), not a transcription: the
// reference builds GLM 3x3 matrices T = W*P and T^T Sigma T; here the 2x2 footprint is
// t_i^T Sigma t_j with t_i = Rv^T u_i the world-space tangent directions (two symmetric
// mat-vecs and three dots), and the backward is written as vector-Jacobian products.
#include "lidargs_common.h"
#include "selection.h"
#include <algorithm>

namespace lg {

__device__ __forceinline__ float3 f3(float x, float y, float z) { return make_float3(x, y, z); }
__device__ __forceinline__ float dot3(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float3 scale3(float3 a, float s) { return f3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float3 add3(float3 a, float3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }

// A v with A[r][k] = view[4r+k]  (= Rv^T v: view-space direction -> world space)
__device__ __forceinline__ float3 view_to_world(const float* vm, float3 v) {
    return f3(vm[0] * v.x + vm[1] * v.y + vm[2] * v.z,
              vm[4] * v.x + vm[5] * v.y + vm[6] * v.z,
              vm[8] * v.x + vm[9] * v.y + vm[10] * v.z);
}
// A^T v (world -> view rotation)
__device__ __forceinline__ float3 world_to_view_dir(const float* vm, float3 v) {
    return f3(vm[0] * v.x + vm[4] * v.y + vm[8] * v.z,
              vm[1] * v.x + vm[5] * v.y + vm[9] * v.z,
              vm[2] * v.x + vm[6] * v.y + vm[10] * v.z);
}

struct Sym3 { float xx, xy, xz, yy, yz, zz; };
__device__ __forceinline__ float3 symmul(const Sym3& S, float3 v) {
    return f3(S.xx * v.x + S.xy * v.y + S.xz * v.z,
              S.xy * v.x + S.yy * v.y + S.yz * v.z,
              S.xz * v.x + S.yz * v.y + S.zz * v.z);
}

// Columns r_k of the standard rotation matrix of quaternion (r,x,y,z); NOT normalised, as the
// reference (R3/cr/forward.cu:228).  Sigma = sum_k s_k^2 r_k r_k^T.
__device__ __forceinline__ void quat_columns(float4 q, float3& c0, float3& c1, float3& c2) {
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    c0 = f3(1.f - 2.f * (y * y + z * z), 2.f * (x * y + r * z), 2.f * (x * z - r * y));
    c1 = f3(2.f * (x * y - r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z + r * x));
    c2 = f3(2.f * (x * z + r * y), 2.f * (y * z - r * x), 1.f - 2.f * (x * x + y * y));
}

__device__ __forceinline__ Sym3 covariance_world(float3 s, float4 q) {
    float3 c0, c1, c2;
    quat_columns(q, c0, c1, c2);
    // rows of M = S R^T are m_k = s_k r_k ; Sigma_ij = sum_k m_k[i] m_k[j]
    float3 m0 = scale3(c0, s.x), m1 = scale3(c1, s.y), m2 = scale3(c2, s.z);
    Sym3 S;
    S.xx = m0.x * m0.x + m1.x * m1.x + m2.x * m2.x;
    S.xy = m0.x * m0.y + m1.x * m1.y + m2.x * m2.y;
    S.xz = m0.x * m0.z + m1.x * m1.z + m2.x * m2.z;
    S.yy = m0.y * m0.y + m1.y * m1.y + m2.y * m2.y;
    S.yz = m0.y * m0.z + m1.y * m1.z + m2.y * m2.z;
    S.zz = m0.z * m0.z + m1.z * m1.z + m2.z * m2.z;
    return S;
}

// Tangent basis at dir (R3/cr/forward.cu:95-119): u1 = normalize(dir.y,-dir.x,0), u2 = dir x u1.
// A zero vector stays zero (poles).
__device__ __forceinline__ void tangent_basis(float3 dir, float3& u1, float3& u2) {
    u1 = f3(dir.y, -dir.x, 0.f);
    float l = sqrtf(u1.x * u1.x + u1.y * u1.y);
    if (l > 0.f) { u1.x /= l; u1.y /= l; }
    u2 = f3(dir.y * u1.z - dir.z * u1.y, dir.z * u1.x - dir.x * u1.z, dir.x * u1.y - dir.y * u1.x);
}

// ------------------------------------------------------------------------------------------------
// entry i of the pixel-ray tables: (cos, sin) of the azimuth of column i and of the elevation of pixel row i
__device__ __forceinline__ void ray_table_entry(int i, const float* __restrict__ beams, int W, int H, float2* __restrict__ coltab,
                                                float2* __restrict__ rowtab) {
    const float pi_f = 3.14159265358979323846f;
    if (i < W) {
        // R3/cr/forward.cu:590: evaluated in double, rounded to float, then float cos/sin
        const double b = -((double)(float)i - (double)(float)W / 2.0) / (double)(float)W * 2.0 * (double)pi_f;
        const float beta = (float)b;
        // float cos/sin of the float angle, evaluated through double so the result is the correctly
        // rounded one (what a good libm returns); the blend differences s - q cancel ~3 digits, so a
        // 1-ulp wobble here is a 1e-5 relative wobble of every per-pair quantity.
        coltab[i] = make_float2((float)cos((double)beta), (float)sin((double)beta));
    }
    if (i < H) {
        const float alp = beams[H - 1 - i];     // R3/cr/forward.cu:589
        rowtab[i] = make_float2((float)cos((double)alp), (float)sin((double)alp));
    }
}
__global__ void k_setup_tables(const float* __restrict__ beams, int W, int H, float2* __restrict__ coltab, float2* __restrict__ rowtab) {
    ray_table_entry(blockIdx.x * blockDim.x + threadIdx.x, beams, W, H, coltab, rowtab);
}

void launch_setup_tables(const float* beams, int W, int H, ImgView img, hipStream_t s) {
    const int n = W > H ? W : H;
    hipLaunchKernelGGL(k_setup_tables, dim3((n + 255) / 256), dim3(256), 0, s, beams, W, H, img.coltab, img.rowtab);
}

// ------------------------------------------------------------------------------------------------
struct PreKernelArgs {
    PreprocessParams pp;
    const float* means3D; const float* scales; const float* rotations; const float* opacities;
    const float* colors; const float* cov3D_precomp; const float* beams;
    int* radii; int* radii_xy;
    float4* rec; uint32_t* rowspan; uint4* spans; uint32_t* dkey; uint32_t* ids;
    uint8_t* touched;                   // [P] "some pixel took this Gaussian" marks of the blend (GeomView::touched): cleared here
    unsigned long long* inst_slots;     // [LG_INST_SLOTS][4]: instance counts for tile heights 4, 8, 16, 32 (zeroed by the caller)
    unsigned long long* diag_slots;     // [LG_INST_SLOTS][2]: visible Gaussians, reference tiles_touched (diagnostics)
    uint32_t* key_span;                 // [LG_INST_SLOTS][2]: ~(smallest), largest range key of the visible Gaussians (zeroed by the caller)
    float2* coltab; float2* rowtab;     // pixel-ray tables for the blend, filled by the first workgroups (nullptr: not wanted)
};

template <bool FILTER>
__global__ void __launch_bounds__(256) k_preprocess(const PreKernelArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const PreprocessParams& pp = a.pp;
    const bool in_range = idx < pp.P;                                  // no early return: the whole wave takes part in the sums at the end
    // a capacity-sized selection's padding rows (enqueue-only rank frames): culled like any other Gaussian -- radius 0, the culled
    // key, empty spans are WRITTEN for them --, but none of their (uninitialised) attributes is read
    const bool row_exists = in_range && (pp.n_valid == nullptr || (uint32_t)idx < *pp.n_valid);
    if (!FILTER && a.coltab) {                                         // W + H table entries ride on the first workgroups: one launch less
        const int n = max(pp.W, pp.H);
        for (int i = idx; i < n; i += gridDim.x * blockDim.x) ray_table_entry(i, a.beams, pp.W, pp.H, a.coltab, a.rowtab);
    }
    // the beam table is binary-searched three times per Gaussian (6 dependent reads each): keep it in LDS when it fits
    constexpr int BEAMS_LDS = 1024;
    __shared__ float s_beams[BEAMS_LDS];
    const bool lds_beams = pp.H <= BEAMS_LDS;
    if (lds_beams) {
        for (int q = threadIdx.x; q < pp.H; q += blockDim.x) s_beams[q] = a.beams[q];
        __syncthreads();
    }
    const float* __restrict__ beams = a.beams;
    auto beam = [&](int q) { return lds_beams ? s_beams[q] : beams[q]; };
    // tan(|beam[i] - beam[i-1]|) of R3/cr/forward.cu:361 depends on the beam interval only: H - 1 values per workgroup instead of
    // one tanf (~60 instructions) per Gaussian; same function on the same argument, so the row radius is bit-identical
    __shared__ float s_tan_gap[BEAMS_LDS];
    if (lds_beams) {
        for (int q = threadIdx.x + 1; q < pp.H; q += blockDim.x) s_tan_gap[q] = tanf(fabsf(s_beams[q] - s_beams[q - 1]));
        __syncthreads();
    }

    int out_radius = 0, rx = 0, ry = 0;
    uint32_t key = 0xFFFFFFFFu, tiles = 0, reftiles = 0, rspan = 0, xsp = 0, t4 = 0, t8 = 0, t16 = 0, t32 = 0;
    float4 r0, r1, r2, r3;
    bool live = false;

    do {
        if (!row_exists) break;
        const float3 pw = f3(a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]);
        const float* vm = pp.view;
        const float3 p = view_point(vm, pw);
        const float dist = range_of(p);
        if (dist >= pp.far_f || dist <= pp.near_f) break;            // R3/cr/forward.cu:304
        if (!in_shell(dist, pp.shell_lo, pp.shell_hi)) break;        // range shell (multi-GPU only): the selection's own test (selection.h)
        // every other input of a surviving Gaussian is requested here, together: the opacity and the colours are needed a thousand
        // instructions further down, where a load issued on the spot would be waited for
        const float op_in = FILTER ? 0.f : a.opacities[idx], col0_in = FILTER ? 0.f : a.colors[2 * idx], col1_in = FILTER ? 0.f : a.colors[2 * idx + 1];   // (K2 has neither)

        Sym3 S;
        if (a.cov3D_precomp) {
            const float* c = a.cov3D_precomp + 6 * (size_t)idx;
            S.xx = c[0]; S.xy = c[1]; S.xz = c[2]; S.yy = c[3]; S.yz = c[4]; S.zz = c[5];
        } else {
            const float m = pp.scale_modifier;
            const float3 sc = f3(m * a.scales[3 * idx], m * a.scales[3 * idx + 1], m * a.scales[3 * idx + 2]);
            const float4 q = make_float4(a.rotations[4 * idx], a.rotations[4 * idx + 1], a.rotations[4 * idx + 2], a.rotations[4 * idx + 3]);
            S = covariance_world(sc, q);
        }

        const float3 dir = f3(p.x / dist, p.y / dist, p.z / dist);
        float3 u1, u2;
        tangent_basis(dir, u1, u2);
        // footprint in the tangent plane: cov_ij = t_i^T Sigma t_j, t_i = world-space tangent
        const float3 t1 = view_to_world(vm, u1), t2 = view_to_world(vm, u2);
        const float3 St1 = symmul(S, t1), St2 = symmul(S, t2);
        const float d2 = dist * dist;
        const float ca = (dot3(t1, St1) + 0.01f) / d2;               // :165-166 low-pass, :319-321 /dist^2
        const float cb = dot3(t1, St2) / d2;
        const float cc = (dot3(t2, St2) + 0.01f) / d2;
        // keep the two cancellation-prone expressions un-contracted so they round as written
        const float det = __fsub_rn(__fmul_rn(ca, cc), __fmul_rn(cb, cb));
        if (det == 0.0f) break;
        const float det_inv = 1.f / det;
        const float conA = cc * det_inv, conB = -cb * det_inv, conC = ca * det_inv;
        const float mid = 0.5f * (ca + cc);
        // :328-330 double max / sqrt (the 1e-9 floor is almost always the active branch)
        // The floor is almost always the active branch of the first max (the footprint's discriminant is O(1e-12)), and sqrt(1e-9)
        // is a constant: the double-precision square root runs only for the lanes (usually none of the wave) above the floor.
        const double xd = (double)__fsub_rn(__fmul_rn(mid, mid), det);
        double disc = 3.1622776601683795e-05;                         // sqrt(1e-9), correctly rounded
        if (xd > 1e-9) disc = sqrt(xd);
        const float lambda1 = (float)((double)mid + disc);
        const float lambda2 = (float)((double)mid - disc);
        // (float)sqrt((double)L) is the correctly rounded fp32 square root of the float L (53 >= 2 * 24 + 2 bits: rounding twice is
        // harmless for sqrt), i.e. sqrtf(L); below the floor it is the constant (float)sqrt(1e-9)
        const float lmax = fmaxf(lambda1, lambda2);
        // (a NaN lmax -- degenerate scales / rotations -- takes the floor like fmax(1e-9, NaN) does in the reference: the test is written
        //  so that the comparison is false for NaN on the sqrt side)
        const float my_radius = !((double)lmax > 1e-9) ? (float)3.1622776601683795e-05 : sqrtf(lmax);

        const float pi_f = 3.14159265358979323846f;
        const float p_c = (pi_f - atan2f(p.y, p.x)) / pp.col_step;  // :333-334
        float alpha;
        if (!FILTER) alpha = atan2f(p.z, sqrtf(p.x * p.x + p.y * p.y));                                           // :336
        else alpha = (float)atan2((double)p.z, sqrt(fmax(1e-9, (double)(p.x * p.x + p.y * p.y))));                // :456

        // beam row: clamp at the ends, else first beam >= alpha (R3/cr/auxiliary.h:41-63)
        const int H = pp.H;
        int bi;
        if (alpha >= beam(H - 1)) bi = H - 1;
        else if (alpha <= beam(0)) bi = 0;
        else {
            int lo = 0, hi = H;
            while (lo < hi) { const int md = (lo + hi) >> 1; if (beam(md) < alpha) lo = md + 1; else hi = md; }
            bi = lo;
        }
        float before, after, p_r;
        const float guard = 0.002f * 2;                                // Ray_Divergence_Angle*2, :22/:347/:356
        const int gap = bi > 0 ? bi : 1;                               // the interval (gap - 1, gap) whose width scales the row radius
        if (bi > 0) {
            before = beam(bi - 1); after = beam(bi);
            p_r = (float)(bi - 1) + (alpha - before) / (after - before);
            if (alpha > (after + guard)) break;
        } else {
            before = beam(0); after = beam(1);
            p_r = (float)(bi + 1) + (alpha - after) / (after - before);
            if (alpha < (before - guard)) break;
        }
        p_r = (float)H - p_r - 1.f;                                    // :359

        ry = (int)ceilf(3.f * my_radius / (lds_beams ? s_tan_gap[gap] : tanf(fabsf(after - before))));   // :361
        rx = (int)ceilf(3.f * my_radius / pp.tan_col_step);            // :362

        // reference rect in 16x1 tiles (R3/cr/auxiliary.h:80-92); x truncates, y rounds
        const int gx = pp.tiles_x, gy = H;
        int xmin, ymin, xmax, ymax;
        rect_lidar(p_c, p_r, rx, ry, gx, gy, xmin, ymin, xmax, ymax);
        if ((xmax - xmin) * (ymax - ymin) == 0) break;

        live = true;
        out_radius = max(rx, ry);
        if (FILTER) break;

        reftiles = (uint32_t)((xmax - xmin) * (ymax - ymin));
        key = __float_as_uint(dist);

        // ---- conservative footprint pruning ------------------------------------------------------
        // The reference rect is 3*sqrt(lambda) with lambda floored at mid + sqrt(1e-9) (:328-330), which
        // inflates far/small Gaussians 2-3x per axis.  A pixel inside that rect still SKIPS the Gaussian
        // unless alpha = opacity*exp(power) >= 1/255 (:606), i.e. unless d^T Q d <= 2 tau, tau = ln(255 o).
        // The axis-aligned extent of that ellipse is |d.x| <= hx = sqrt(2 tau cov_xx), |d.y| <= hy = sqrt(2 tau cov_yy),
        // and for the tangent basis used here (u1 = azimuthal, u2 = -d/d elevation) the offsets of the pixel at
        // (beta, alpha) from the centre (beta0, alpha0) are EXACTLY
        //     d.x = cos(alpha) sin(beta - beta0)
        //     d.y = sin(alpha - alpha0) + cos(alpha) sin(alpha0) (1 - cos(beta - beta0)).
        // Hence a taking pixel needs |sin dbeta| <= hx / cos(alpha) and |sin dalpha| <= hy + |sin alpha0| (1 - cos dbeta_max):
        // an axis-aligned bound in (column, row) that follows the footprint's anisotropy.  Tiles / rows outside it
        // are dropped from the lists without changing any pixel; the margins cover float rounding.
        int tx0 = xmin, tx1 = xmax, ty_lo = ymin, ty_hi = ymax;
        const float op = op_in;
        // The bounds below turn |sin(dbeta)| <= sb into |dbeta| <= asin(sb), which holds on [0, pi/2] only.  The reference evaluates the
        // Gaussian at EVERY pixel of the 16-column tiles its rect touches, and a pixel looking the other way (dbeta near pi) has
        // sin(dbeta) near 0 again: delta = pixel_dir - dir projects onto the tangent plane as (0, 0) at the antipode, so the reference
        // blends the Gaussian there at full weight.  With W <= 32 a single tile spans that far (found by tools/parity_sweep.py on W = 25:
        // a Gaussian at column 12.5 contributing at column 0), with a footprint wider than a quarter of the panorama the rect does.  Such
        // Gaussians keep their whole reference rect; so does every Gaussian of a beam fan wider than pi/2 (same argument for the rows).
        const float reach = fmaxf(p_c - 16.f * (float)xmin, 16.f * (float)xmax - p_c) * pp.col_step;
        const bool small_angles = reach < 1.5f && (beam(H - 1) - beam(0)) < 1.5f;
        if (op * 255.f < 1.f) { tx1 = tx0; }                           // can never reach 1/255 (a NaN opacity passes: min(0.99, NaN) is 0.99 in the blend)
        else if (pp.prune && small_angles) {
            // Everything here is a bound from above, so the cheap forms are as safe as the exact ones: the hardware log (the
            // 0.02 covers its error), asin(x) <= x + 0.23 x^3 on [0, 0.7], 1 - cos(t) <= t^2 / 2, |sin(alpha)| = |dir.z|.
            const float tau2 = 2.f * (__logf(255.f * op) + 0.02f);
            const float hx = sqrtf(tau2 * ca) * 1.002f + 1e-6f, hy = sqrtf(tau2 * cc) * 1.002f + 1e-6f;
            // smallest cos(elevation) of any pixel row, from below: cos(b) >= 1 - b^2 / 2 at the two ends of the fan (two cosf
            // calls were ~100 of each thread's ~1400 instructions); a fan reaching past ~70 degrees gives up the column bound
            const float b_lo = beam(0), b_hi = beam(H - 1);
            const float cfan = (1.f - 0.5f * fmaxf(b_lo * b_lo, b_hi * b_hi)) * 0.999f;
            const float sb = cfan > 0.05f ? hx * (__builtin_amdgcn_rcpf(cfan) * 1.00001f) : 1.f;   // bound on |sin(dbeta)|
            float one_m_cos = 2.f;                                     // 1 - cos(dbeta_max): worst case if unbounded
            if (sb < 0.7f) {
                const float dbeta = (sb + 0.23f * sb * sb * sb) * 1.002f + 2e-5f;
                one_m_cos = 0.5f * dbeta * dbeta * 1.000001f + 1e-7f;
                const float dcol = dbeta * pp.inv_col_step + 0.02f;    // pixel x is reachable iff |x - p_c| <= dcol
                tx0 = max(tx0, (int)floorf((p_c - dcol) / 16.f));
                tx1 = min(tx1, (int)floorf((p_c + dcol) / 16.f) + 1);
            }
            const float sa = hy + (fabsf(dir.z) * 1.00001f + 1e-7f) * one_m_cos;     // bound on |sin(dalpha)|
            if (sa < 0.7f) {
                const float dalpha = (sa + 0.23f * sa * sa * sa) * 1.002f + 2e-5f;
                const float e_lo = alpha - dalpha, e_hi = alpha + dalpha;
                int lo = 0, hi = H;                                    // first beam >= e_lo
                while (lo < hi) { const int md = (lo + hi) >> 1; if (beam(md) < e_lo) lo = md + 1; else hi = md; }
                const int i_lo = lo;
                lo = 0; hi = H;                                        // first beam > e_hi
                while (lo < hi) { const int md = (lo + hi) >> 1; if (beam(md) <= e_hi) lo = md + 1; else hi = md; }
                const int i_hi = lo;                                   // beams [i_lo, i_hi) are in reach
                ty_lo = max(ty_lo, H - i_hi);                          // pixel row y = H-1-i
                ty_hi = min(ty_hi, H - i_lo);
            }
        }
        tx0 = max(tx0, pp.tile_x_lo); tx1 = min(tx1, pp.tile_x_hi);    // column wedge (multi-GPU): other ranks bin the other tile columns
        if (tx1 <= tx0 || ty_hi <= ty_lo) { tiles = 0; tx0 = tx1 = xmin; ty_lo = ty_hi = ymin; }
        else {
            tiles = (uint32_t)(tx1 - tx0);                              // tile columns; the rows depend on the tile height chosen later
            t4 = tiles * (uint32_t)((ty_hi - 1) / 4 - ty_lo / 4 + 1);
            t8 = tiles * (uint32_t)((ty_hi - 1) / 8 - ty_lo / 8 + 1);
            t16 = tiles * (uint32_t)((ty_hi - 1) / 16 - ty_lo / 16 + 1);
            t32 = tiles * (uint32_t)((ty_hi - 1) / 32 - ty_lo / 32 + 1);
        }
        rspan = (uint32_t)ty_lo | ((uint32_t)ty_hi << 16);
        xsp = (uint32_t)tx0 | ((uint32_t)tx1 << 16);
        if (!tiles) key = 0xFFFFFFFFu;                                 // binned nowhere: sorted with the culled ones (no instances either way)

        // scaled bases: d.x = delta.u1 / (u1.u1) == delta.u1'  (R3/cr/forward.cu:593-597)
        const float uu1 = dot3(u1, u1), uu2 = dot3(u2, u2);
        const float i1 = uu1 > 0.f ? 1.f / uu1 : 0.f, i2 = uu2 > 0.f ? 1.f / uu2 : 0.f;
        r0 = make_float4(dir.x, dir.y, dir.z, dist);
        r1 = make_float4(u1.x * i1, u2.x * i2, u1.y * i1, u2.y * i2);                  // (u1', u2') interleaved by component:
        r2 = make_float4(u1.z * i1, u2.z * i2, conA, conC);                            // the blend evaluates both projections in
        r3 = make_float4(conB, op_in, col0_in, col1_in);   // packed-fp32 operations
    } while (false);

    if (in_range) {
        a.radii[idx] = out_radius;
        if (a.radii_xy) { a.radii_xy[2 * idx] = live ? rx : 0; a.radii_xy[2 * idx + 1] = live ? ry : 0; }  // every row written: callers need not pre-zero; NULL: not wanted
    }
    if (FILTER) return;
    {   // instance totals for tile heights 4 / 8 / 16 / 32 (the host picks the height from them, api.hip choose_tile_rows): one block
        // sum, added to one of LG_INST_SLOTS slots -- 31 k waves adding to the same three words cost a millisecond, 7.8 k blocks
        // spread over 64 lines do not show; the host adds the slots up after its one read
        // (two more sums ride along for lidargs_last_counters: the visible Gaussians and the reference's 16x1 tiles_touched)
        __shared__ uint32_t s_part[4][8];
        uint32_t s4 = t4, s8 = t8, s16 = t16, s32 = t32, sv = reftiles ? 1u : 0u, sr = reftiles;
        // ~(smallest) and largest range key of the block's visible Gaussians (key = 0xFFFFFFFF: culled -> neutral for both maxima)
        uint32_t kinv = ~key, kmx = (key == 0xFFFFFFFFu) ? 0u : key;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s4 += __shfl_xor(s4, o); s8 += __shfl_xor(s8, o); s16 += __shfl_xor(s16, o); s32 += __shfl_xor(s32, o);
            sv += __shfl_xor(sv, o); sr += __shfl_xor(sr, o);
            kinv = max(kinv, (uint32_t)__shfl_xor((int)kinv, o)); kmx = max(kmx, (uint32_t)__shfl_xor((int)kmx, o));
        }
        if ((threadIdx.x & 63) == 0) {
            uint32_t* q = s_part[threadIdx.x >> 6];
            q[0] = s4; q[1] = s8; q[2] = s16; q[3] = s32; q[4] = sv; q[5] = sr; q[6] = kinv; q[7] = kmx;
        }
        __syncthreads();
        if (threadIdx.x == 6 || threadIdx.x == 7) {
            const int c = threadIdx.x;
            const uint32_t m = max(max(s_part[0][c], s_part[1][c]), max(s_part[2][c], s_part[3][c]));
            // (a plain look at the slot first, to skip the atomic when it would change nothing, cost 14 us of this launch: the load has to
            //  come back before the block can retire, the atomic does not)
            if (m) atomicMax(a.key_span + 2 * (size_t)(blockIdx.x % LG_INST_SLOTS) + (c - 6), m);
        }
        if (threadIdx.x < 6) {
            const uint32_t sum = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
            const size_t slot = (size_t)(blockIdx.x % LG_INST_SLOTS);
            if (sum) {
                if (threadIdx.x < 4) atomicAdd(a.inst_slots + slot * 4 + threadIdx.x, (unsigned long long)sum);
                else atomicAdd(a.diag_slots + slot * 2 + (threadIdx.x - 4), (unsigned long long)sum);
            }
        }
    }
    // The backward blend adds into the packed 64-byte gradient line of a Gaussian.  Rounds 2-4 zeroed all P lines here (64 B x P: 128 of
    // this launch's 420 MB at 2 M Gaussians).  Only the Gaussians some pixel's walk takes -- a third of the visible ones on the street
    // frames -- are ever added to: the blend marks them (one byte each, cleared here), and the backward's first launch clears exactly
    // their lines (k_zero_touched).
    if (!in_range) return;
    a.touched[idx] = 0;
    a.dkey[idx] = key;
    // an empty column span = no instances, whatever the row span holds
    if (pp.compact) reinterpret_cast<uint32_t*>(a.spans)[idx] = span_pack(rspan, tiles ? xsp : 0u);
    else a.spans[idx] = make_uint4(rspan, tiles ? xsp : 0u, 0u, 0u);
    if (live && tiles) {                                               // (only binned Gaussians' records are ever gathered)
        a.rowspan[idx] = rspan;
        float4* r = a.rec + 4 * (size_t)idx;
        r[0] = r0; r[1] = r1; r[2] = r2; r[3] = r3;
    }
}

void launch_preprocess(const PreprocessParams& pp, const float* means3D, const float* scales, const float* rotations,
                       const float* opacities, const float* colors, const float* cov3D_precomp, const float* beams,
                       int* radii, int* radii_xy, GeomView g, const ImgView* tables, bool filter_only, hipStream_t s) {
    PreKernelArgs a;
    a.pp = pp;
    a.means3D = means3D; a.scales = scales; a.rotations = rotations; a.opacities = opacities; a.colors = colors;
    a.cov3D_precomp = cov3D_precomp; a.beams = beams; a.radii = radii; a.radii_xy = radii_xy;
    a.coltab = tables ? tables->coltab : nullptr; a.rowtab = tables ? tables->rowtab : nullptr;
    a.rec = g.rec; a.rowspan = g.rowspan; a.spans = g.spans; a.dkey = g.key_a; a.ids = g.id_a;
    a.touched = g.touched;
    a.inst_slots = reinterpret_cast<unsigned long long*>(g.totals + LG_TOTALS_SLOT_WORD);
    a.diag_slots = reinterpret_cast<unsigned long long*>(g.totals + LG_TOTALS_DIAG_WORD);
    a.key_span = g.totals + LG_TOTALS_KEYSPAN_WORD;
    const dim3 grid((pp.P + 255) / 256), block(256);
    if (filter_only) hipLaunchKernelGGL(k_preprocess<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_preprocess<false>, grid, block, 0, s, a);
}

// ------------------------------------------------------------------------------------------------
__global__ void k_mark_visible(int P, const float* __restrict__ means3D, const float* __restrict__ vm, unsigned char* __restrict__ present) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const float x = means3D[3 * i], y = means3D[3 * i + 1], z = means3D[3 * i + 2];
    const float vz = vm[2] * x + vm[6] * y + vm[10] * z + vm[14];
    present[i] = (vz <= 0.2f) ? 0 : 1;      // R3/cr/auxiliary.h:190
}

void launch_mark_visible(int P, const float* means3D, const float* view, unsigned char* present, hipStream_t s) {
    hipLaunchKernelGGL(k_mark_visible, dim3((P + 255) / 256), dim3(256), 0, s, P, means3D, view, present);
}

// Test hook (lidargs_debug_rects): the rect arithmetic of the two preprocess kernels on caller-supplied (p_c, p_r, rx, ry), so that
// tests can put millions of inputs within an ulp of every truncation / rounding boundary -- one random Gaussian in 1e8 lands there.
__global__ void k_debug_rects(int n, int surfel, const float2* __restrict__ p, const int2* __restrict__ r, int gx, int gy, int4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int xmin, ymin, xmax, ymax;
    if (surfel) rect_surfel(p[i].x, p[i].y, r[i].x, r[i].y, gx, gy, xmin, ymin, xmax, ymax);
    else rect_lidar(p[i].x, p[i].y, r[i].x, r[i].y, gx, gy, xmin, ymin, xmax, ymax);
    out[i] = make_int4(xmin, ymin, xmax, ymax);
}
void launch_debug_rects(int n, int surfel, const float* p_cr, const int* r_xy, int gx, int gy, int* rects, hipStream_t s) {
    k_debug_rects<<<(n + 255) / 256, 256, 0, s>>>(n, surfel, (const float2*)p_cr, (const int2*)r_xy, gx, gy, (int4*)rects);
}

// ------------------------------------------------------------------------------------------------
// K9 + K10 fused.  Inputs are the per-Gaussian sums the backward blend produced (gacc, 64 B per
// Gaussian): dL/dconic (A,B,C), the moments G1, G2 of dL/du1, dL/du2 (direct part), (gx,gy) = dL/dmean2D.xy, dL/drange,
// dL/dopacity, dL/dcolour.  dL/dsphere is NOT accumulated per pixel: by linearity it equals
//   gx*u1' + gy*u2' (R3/cr/backward.cu:759-777 sums exactly these per-pixel terms).
//
// Sparse (round 5).  A gradient exists only for the Gaussians the blend marked as touched -- on the street frames a fifth of the visible
// ones (0.33 of 1.73 M); everybody else's rows are zero (K9 / K10 are linear in the sums, R3/cr/backward.cu:453-532; the reference gets
// the same zeros from torch::zeros, R3/rasterize_points.cu:163-175).  The backward's first launch (k_zero_touched below) zeroes all
// rows and lists the touched Gaussians region by region; k_gaussian_backward runs the chain on the listed ones only and overwrites
// their rows.  An untouched Gaussian costs its mark and 68 bytes of zeros: no inputs, no radius, no 64-byte line.
// the chain of one touched Gaussian.  POSE (the pose form, k_gaussian_backward_view below): the row's twelve products of dL/dviewmatrix are
// added to the lane's running sums ps[16] as well (slot 4r + k = element [r][k] of the matrix; slots 3, 7, 11, 15 stay zero)
template <bool POSE = false>
__device__ __forceinline__ void gb_row(const GaussBwdArgs& a, const int idx, float* ps = nullptr) {
#pragma clang fp contract(fast)                                        // (see below, behind the early return)
    const float* vm = a.view;

    // every input of the row is requested here, together (one round trip for the wave instead of three: the loads behind the early
    // return and behind the covariance were issued where they stand in the text)
    const float3 pw = get3(a.means3D, idx);
    const float4* acc = reinterpret_cast<const float4*>(a.gacc) + 4 * (size_t)idx;
#if defined(LG_GB_VARIANT) && LG_GB_VARIANT == 7    /* experiment: no packed-line loads */
    const float ff = (float)(idx & 255);
    const float4 q0 = make_float4(ff, 1.f, 2.f, ff), q1 = q0, q2 = q0, q3 = q0;
#else
    float4 q0 = acc[0], q1 = acc[1], q2 = acc[2], q3 = acc[3];
#endif
    if (a.det_mode && (*a.det_mode & LG_MODE_DETERMINISTIC) != 0u) {
        // deterministic buffers (lidargs_common.h "deterministic accumulation"): the float line holds each slot's largest term, the
        // sums are the 64-bit line's, read on the grid that term fixes
        const longlong2* w = reinterpret_cast<const longlong2*>(a.acc64 + 16 * (size_t)idx);
        auto line = [&](float4& q, int k) {
            const longlong2 lo = w[2 * k], hi = w[2 * k + 1];
            q = make_float4(det_decode(__float_as_uint(q.x), lo.x), det_decode(__float_as_uint(q.y), lo.y),
                            det_decode(__float_as_uint(q.z), hi.x), det_decode(__float_as_uint(q.w), hi.y));
        };
        line(q0, 0); line(q1, 1); line(q2, 2); line(q3, 3);
    }
    const bool have_sr = (a.cov3D_precomp == nullptr);
    float3 s_in = f3(0, 0, 0); float4 q = make_float4(1, 0, 0, 0);
    float3 cv0 = f3(0, 0, 0), cv1 = f3(0, 0, 0);
    if (have_sr || a.scales) { s_in = get3(a.scales, idx); q = get4(a.rotations, idx); }
    if (!have_sr) { cv0 = get3(a.cov3D_precomp, 2 * (size_t)idx); cv1 = get3(a.cov3D_precomp, 2 * (size_t)idx + 1); }
    const float3 d = f3(vm[0] * pw.x + vm[4] * pw.y + vm[8] * pw.z + vm[12],
                        vm[1] * pw.x + vm[5] * pw.y + vm[9] * pw.z + vm[13],
                        vm[2] * pw.x + vm[6] * pw.y + vm[10] * pw.z + vm[14]);
    const float n2 = d.x * d.x + d.y * d.y + d.z * d.z;
    const float dist = __builtin_amdgcn_sqrtf(n2);
    if (dist <= 0.f) return;                                           // R3/cr/backward.cu:488 (the rows are zero already)
    // Everything below is a gradient: held to 1e-4, not to the last bit, and this launch's length follows its instruction count (31 M
    // vector instructions: 51 of its 78 us at the clock's nominal rate).  The file is built without contraction for K1's cancelling
    // footprint expressions; here multiply-adds fuse (the one cancelling product difference, `denom`, is written with explicit rounding
    // steps), the divisions are a reciprocal + one residual correction (four instructions for the IEEE sequence's ten), the square roots
    // the hardware's.
    auto frcp = [](float b) { const float r = __builtin_amdgcn_rcpf(b); return __builtin_fmaf(__builtin_fmaf(-b, r, 1.f), r, r); };
    const float inv_dist = frcp(dist);
    const float3 dir = f3(d.x * inv_dist, d.y * inv_dist, d.z * inv_dist);
    float3 u1, u2;
    tangent_basis(dir, u1, u2);

    Sym3 S;
    const float3 sc = f3(a.scale_modifier * s_in.x, a.scale_modifier * s_in.y, a.scale_modifier * s_in.z);
    if (!have_sr) { S.xx = cv0.x; S.xy = cv0.y; S.xz = cv0.z; S.yy = cv1.x; S.yz = cv1.y; S.zz = cv1.z; }
    else S = covariance_world(sc, q);
    const float3 t1 = view_to_world(vm, u1), t2 = view_to_world(vm, u2);
    const float3 St1 = symmul(S, t1), St2 = symmul(S, t2);
    const float _a = dot3(t1, St1) + 0.01f, _b = dot3(t1, St2), _c = dot3(t2, St2) + 0.01f;
    const float inv_d2 = frcp(dist * dist);
    const float ca = inv_d2 * _a, cb = inv_d2 * _b, cc = inv_d2 * _c;

    // unpack the blend kernel's packed sums into the caller's arrays (the reference accumulates
    // straight into them with atomics, R3/cr/backward.cu:702-788)
    const float gx = q0.x, gy = q0.y;
    const float gA = q0.w, gB = q1.x, gC = q1.y;
    const float gdep = q2.y;
    // slots 10-15 hold the moment vectors G1 = sum_pixels gx delta, G2 = sum gy delta; the direct basis gradients the reference
    // accumulates per pixel (R3/cr/backward.cu:738-750) are  du_i = |u_i'|^2 G_i - 2 u_i' (u_i' . G_i),  u_i' = u_i / (u_i . u_i)
    float3 du1, du2;
    {
        const float w1 = dot3(u1, u1), w2 = dot3(u2, u2);
        const float j1 = w1 > 0.f ? frcp(w1) : 0.f, j2 = w2 > 0.f ? frcp(w2) : 0.f;
        const float3 G1 = f3(q2.z, q2.w, q3.x), G2 = f3(q3.y, q3.z, q3.w);
        const float3 p1 = scale3(u1, j1), p2 = scale3(u2, j2);
        const float c1 = 2.f * dot3(p1, G1), c2 = 2.f * dot3(p2, G2);
        du1 = f3(j1 * G1.x - c1 * p1.x, j1 * G1.y - c1 * p1.y, j1 * G1.z - c1 * p1.z);
        du2 = f3(j2 * G2.x - c2 * p2.x, j2 * G2.y - c2 * p2.y, j2 * G2.z - c2 * p2.z);
    }
    put4(a.dL_dmean2D, idx, gx, gy, q0.z, 0.f);
    // the reference's scratch gradients (conic, depth, sphere, basis) are materialised only if the caller wants them
    if (a.dL_dconic) put4(a.dL_dconic, idx, gA, gB, 0.f, gC);
    a.dL_dopacity[idx] = q1.z;
    put2(a.dL_dcolor, idx, q1.w, q2.x);
    if (a.dL_ddepths) a.dL_ddepths[idx] = gdep;
    if (a.dL_dbasis_u1) put3(a.dL_dbasis_u1, idx, du1.x, du1.y, du1.z);
    if (a.dL_dbasis_u2) put3(a.dL_dbasis_u2, idx, du2.x, du2.y, du2.z);

    // conic -> covariance, with the reference's 1/(denom^2 + 1e-7) damping (R3/cr/backward.cu:237)
    const float denom = __fsub_rn(__fmul_rn(ca, cc), __fmul_rn(cb, cb));
    const float k = frcp((denom * denom) + 0.0000001f);
    float da = k * (-cc * cc * gA + 2.f * cb * cc * gB + (denom - ca * cc) * gC);
    float dc = k * (-ca * ca * gC + 2.f * ca * cb * gB + (denom - ca * cc) * gA);
    float db = k * 2.f * (cb * cc * gA - (denom + 2.f * cb * cb) * gB + ca * cb * gC);
    // range dependence of the /dist^2 factor (:249-252)
    const float dist4 = n2 * n2;
    const float wsum = -2.f * (da * _a + db * _b + dc * _c) * frcp(dist4);
    float3 g_mean = f3(wsum * d.x, wsum * d.y, wsum * d.z);
    da *= inv_d2; dc *= inv_d2; db *= inv_d2;                         // :254-256

    // dL/dSigma, packed upper triangle with doubled off-diagonals (:262-272)
    const float S00 = t1.x * t1.x * da + t1.x * t2.x * db + t2.x * t2.x * dc;
    const float S11 = t1.y * t1.y * da + t1.y * t2.y * db + t2.y * t2.y * dc;
    const float S22 = t1.z * t1.z * da + t1.z * t2.z * db + t2.z * t2.z * dc;
    const float S01 = 2.f * t1.x * t1.y * da + (t1.x * t2.y + t1.y * t2.x) * db + 2.f * t2.x * t2.y * dc;
    const float S02 = 2.f * t1.x * t1.z * da + (t1.x * t2.z + t1.z * t2.x) * db + 2.f * t2.x * t2.z * dc;
    const float S12 = 2.f * t1.z * t1.y * da + (t1.y * t2.z + t1.z * t2.y) * db + 2.f * t2.y * t2.z * dc;
    if (a.dL_dcov3D) { put3(a.dL_dcov3D, 2 * (size_t)idx, S00, S01, S02); put3(a.dL_dcov3D, 2 * (size_t)idx + 1, S11, S12, S22); }   // NULL: only the scale / rotation path wants it

    // dL/dt_i = 2 (Sigma t_i) d{a,c} + (Sigma t_j) db ; dL/du_i = A^T dL/dt_i + direct part (:281-307)
    const float3 gt1 = add3(scale3(St1, 2.f * da), scale3(St2, db));
    const float3 gt2 = add3(scale3(St2, 2.f * dc), scale3(St1, db));
    float3 gu1 = world_to_view_dir(vm, gt1), gu2 = world_to_view_dir(vm, gt2);
    gu1.x += du1.x; gu1.y += du1.y;
    gu2.x += du2.x; gu2.y += du2.y; gu2.z += du2.z;

    // basis -> dir, with the reference's double epsilons (:336-354)
    const float rho2 = dir.x * dir.x + dir.y * dir.y;
    // (the reference's epsilons are doubles: the sum is formed in double, its reciprocal in float)
    const float srho = __builtin_amdgcn_sqrtf(rho2);
    const float i32 = frcp((float)((double)(srho * srho * srho) + 1e-9));
    const float irho = frcp((float)((double)srho + 1e-9));
    float3 gdir;
    gdir.x = i32 * (-dir.y * dir.x * gu1.x - dir.y * dir.y * gu1.y + dir.z * dir.y * dir.y * gu2.x - dir.x * dir.y * dir.z * gu2.y) - dir.x * irho * gu2.z;
    gdir.y = i32 * (dir.x * dir.x * gu1.x + dir.x * dir.y * gu1.y - dir.x * dir.y * dir.z * gu2.x + dir.z * dir.x * dir.x * gu2.y) - dir.y * irho * gu2.z;
    gdir.z = irho * (dir.x * gu2.x + dir.y * gu2.y);
    // dir -> d : (|d|^2 I - d d^T) / (|d|^3 + 1e-9)  (:312-333)
    const float d3 = dist * dist * dist;
    const float id3e = frcp((float)((double)d3 + 1e-9));
    const float dg = dot3(d, gdir);
    g_mean = add3(g_mean, scale3(f3(n2 * gdir.x - d.x * dg, n2 * gdir.y - d.y * dg, n2 * gdir.z - d.z * dg), id3e));

    // K10: sphere-mean and range terms (R3/cr/backward.cu:490-522)
    const float uu1 = dot3(u1, u1), uu2 = dot3(u2, u2);
    const float i1 = uu1 > 0.f ? frcp(uu1) : 0.f, i2 = uu2 > 0.f ? frcp(uu2) : 0.f;
    const float3 gs = add3(scale3(u1, gx * i1), scale3(u2, gy * i2));
    if (a.dL_dsphere) put3(a.dL_dsphere, idx, gs.x, gs.y, gs.z);
    const float id3 = frcp(d3);
    const float dgs = dot3(d, gs);
    float3 v;
    v.x = g_mean.x + (n2 * gs.x - d.x * dgs) * id3 + gdep * dir.x;
    v.y = g_mean.y + (n2 * gs.y - d.y * dgs) * id3 + gdep * dir.y;
    v.z = g_mean.z + (n2 * gs.z - d.z * dgs) * id3 + gdep * dir.z;
    const float3 gw = view_to_world(vm, v);                            // transformVec4x3Transpose (:525)
    put3(a.dL_dmean3D, idx, gw.x, gw.y, gw.z);
    if constexpr (POSE) {
        // The matrix enters K1 twice: d[k] = sum_r vm[4r+k] pw[r] + vm[12+k] and t_i[r] = sum_k vm[4r+k] u_i[k].  v is the gradient
        // on d, gt_i the one on t_i (the values world_to_view_dir was handed above), so this row's share of dL/dvm[4r+k] is
        // v[k] pw[r] + gt1[r] u1[k] + gt2[r] u2[k], and of dL/dvm[12+k] it is v[k].
        const float pr[3] = {pw.x, pw.y, pw.z}, vk[3] = {v.x, v.y, v.z};
        const float g1[3] = {gt1.x, gt1.y, gt1.z}, g2[3] = {gt2.x, gt2.y, gt2.z};
        const float a1[3] = {u1.x, u1.y, u1.z}, a2[3] = {u2.x, u2.y, u2.z};
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int k = 0; k < 3; k++) ps[4 * r + k] += vk[k] * pr[r] + g1[r] * a1[k] + g2[r] * a2[k];
#pragma unroll
        for (int k = 0; k < 3; k++) ps[12 + k] += vk[k];
    }

    if (!a.scales) {
        put3(a.dL_dscale, idx, 0.f, 0.f, 0.f);
        put4(a.dL_drot, idx, 0.f, 0.f, 0.f, 0.f);
    } else {
        // Sigma = sum_k s_k^2 r_k r_k^T, G = symmetric gradient (off-diagonals halved, :415-419)
        Sym3 G; G.xx = S00; G.xy = 0.5f * S01; G.xz = 0.5f * S02; G.yy = S11; G.yz = 0.5f * S12; G.zz = S22;
        float3 c0, c1, c2;
        quat_columns(q, c0, c1, c2);
        const float3 h0 = symmul(G, c0), h1 = symmul(G, c1), h2 = symmul(G, c2);
        // dL/ds_k = 2 s_k r_k^T G r_k  (w.r.t. the MODIFIED scale, as the reference, :428-432)
        put3(a.dL_dscale, idx, 2.f * sc.x * dot3(c0, h0), 2.f * sc.y * dot3(c1, h1), 2.f * sc.z * dot3(c2, h2));
        // F[k][c] = dL/dR[c][k] = 2 s_k^2 (G r_k)[c]
        const float3 F0 = scale3(h0, 2.f * sc.x * sc.x), F1 = scale3(h1, 2.f * sc.y * sc.y), F2 = scale3(h2, 2.f * sc.z * sc.z);
        const float F00 = F0.x, F01 = F0.y, F02 = F0.z, F10 = F1.x, F11 = F1.y, F12 = F1.z, F20 = F2.x, F21 = F2.y, F22 = F2.z;
        const float r = q.x, x = q.y, y = q.z, z = q.w;
        // :440-447, no normalisation Jacobian
        put4(a.dL_drot, idx, 2.f * z * (F01 - F10) + 2.f * y * (F20 - F02) + 2.f * x * (F12 - F21),
             2.f * y * (F10 + F01) + 2.f * z * (F20 + F02) + 2.f * r * (F12 - F21) - 4.f * x * (F22 + F11),
             2.f * x * (F10 + F01) + 2.f * r * (F20 - F02) + 2.f * z * (F12 + F21) - 4.f * y * (F22 + F00),
             2.f * r * (F01 - F10) + 2.f * x * (F20 + F02) + 2.f * y * (F12 + F21) - 4.f * z * (F11 + F00));
    }
}

// One WAVE per region of LG_REGION consecutive Gaussians: the region's touched ones were listed by k_zero_touched (region-local
// offsets, their count), and the wave runs the chain on them, 64 at a time.  Every wave of the launch has work of the same kind: with
// the list compacted inside a 256-thread block instead (one wave of four working, ~40 of its lanes), a block lived as long as that
// one wave's three memory round trips and the launch took 77 us for 0.33 M rows (tools/micro/gauss_bwd_bench.cpp).
__global__ void __launch_bounds__(256) k_gaussian_backward(const GaussBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int region = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int base = region * LG_REGION;
    if (base >= a.P) return;
    // the list slot with the count, not behind it (the list is padded: any slot may be read).  Left to itself the compiler sinks the slot's
    // load below the test on the count -- two round trips where one does --, so both values pass through an empty asm statement
    int off = (int)a.tlist[base + lane];
    int cnt = (int)a.tcount[region];
    asm volatile("" : "+v"(off), "+v"(cnt));
    for (int j = lane; j < cnt; j += 64) {
        gb_row(a, base + off);
        if (j + 64 < cnt) off = (int)a.tlist[base + j + 64];
    }
}

// The pose form of the launch above (lgpose_backward_view): the same chain on the same lists, and the gradient with respect to the
// view matrix on top.  A lane adds the twelve products of its rows (at most LG_REGION / 64 = 4 of them, in list order) to running sums;
// the wave folds the sums over its 64 lanes in a fixed order -- two gfx950 lane swaps, then DPP row rotations and quad permutes -- and
// writes them as the region's 64-byte partial row: view_partials[16 region + 4r + k], zeros in column 3.  Every region of the launch
// writes its row (zeros where nothing was touched), so the buffer need not be cleared.  No atomics: given the same packed lines the rows
// are the same bits whatever the order the waves run in.
__global__ void __launch_bounds__(256) k_gaussian_backward_view(const GaussBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int region = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int base = region * LG_REGION;
    if (base >= a.P) return;
    int off = (int)a.tlist[base + lane];
    int cnt = (int)a.tcount[region];
    asm volatile("" : "+v"(off), "+v"(cnt));
    float ps[16];
#pragma unroll
    for (int k = 0; k < 16; k++) ps[k] = 0.f;
    for (int j = lane; j < cnt; j += 64) {
        gb_row<true>(a, base + off, ps);
        if (j + 64 < cnt) off = (int)a.tlist[base + j + 64];
    }
    // (every lane of the wave is here again: the loop's trip count differs between lanes, the reduction below is wave-wide)
    // halves of 32, then of 16: lane L is left with slots 4 (L >> 4) .. 4 (L >> 4) + 3 in ps[0..3], i.e. row L >> 4 of the matrix
#pragma unroll
    for (int k = 0; k < 8; k++) ps[k] = fold_halves32(ps[k], ps[k + 8]);
#pragma unroll
    for (int k = 0; k < 4; k++) ps[k] = fold_halves16(ps[k], ps[k + 4]);
    // the sixteen lanes of a row hold partial sums of the same four slots: rotations by 8 and 4, then the quad's lanes 2 and 1 apart
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float x = ps[k];
        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xF, 0xF, true));   // row_ror:8
        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124, 0xF, 0xF, true));   // row_ror:4
        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
        ps[k] = x;
    }
    // lanes 0, 16, 32, 48 store the four 16-byte quarters of the region's line with one instruction
    if ((lane & 15) == 0)
        reinterpret_cast<float4*>(a.view_partials)[4 * (size_t)region + (lane >> 4)] = make_float4(ps[0], ps[1], ps[2], ps[3]);
}

// The second launch of the pose form: the partial rows folded into dL_dviewmatrix[16] in double, in a fixed order.  One workgroup;
// thread (g, e) = (tid / 16, tid % 16) adds element e of rows g, g + 64, g + 128, ... in ascending order, thread e < 16 then adds the 64
// group sums in ascending g and rounds once.  All sixteen outputs are written; column 3 is a sum of +0s.
constexpr int LG_VIEW_FOLD_GROUPS = 64;
__global__ void __launch_bounds__(16 * LG_VIEW_FOLD_GROUPS) k_fold_view_partials(const float* __restrict__ partials, int rows, float* __restrict__ out) {
    __shared__ double s_sum[LG_VIEW_FOLD_GROUPS][16];
    const int e = threadIdx.x & 15, g = threadIdx.x >> 4;
    double acc = 0.0;
    int r = g;
    for (; r + 7 * LG_VIEW_FOLD_GROUPS < rows; r += 8 * LG_VIEW_FOLD_GROUPS) {   // eight loads in flight, added in row order
        float x[8];
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = partials[16 * (size_t)(r + i * LG_VIEW_FOLD_GROUPS) + e];
#pragma unroll
        for (int i = 0; i < 8; i++) acc += (double)x[i];
    }
    for (; r < rows; r += LG_VIEW_FOLD_GROUPS) acc += (double)partials[16 * (size_t)r + e];
    s_sum[g][e] = acc;
    __syncthreads();
    if (threadIdx.x < 16) {
        double t = 0.0;
        for (int k = 0; k < LG_VIEW_FOLD_GROUPS; k++) t += s_sum[k][e];
        out[e] = (float)t;
    }
}

// First launch of every backward, one thread per Gaussian, one block per region of LG_REGION:
//   * the packed gradient line of each touched Gaussian is cleared (a second backward on the same forward buffers -- retain_graph --
//     starts from zeroed lines like the first): a wave looks at the marks of its 64 Gaussians (one coalesced 64-byte read) and clears
//     the marked ones' lines LINE float4 at a time, sixteen (eight) lanes per 64-byte (128-byte) line -- whole-line stores, nothing
//     for the unmarked;
//   * the region's touched Gaussians are listed (region-local offsets in index order + their count) for k_gaussian_backward;
//   * every gradient row of every Gaussian is zeroed, whole lines at a time (the reference's torch::zeros, R3/rasterize_points.cu:163-175);
//     k_gaussian_backward then overwrites the touched ones' rows.  (Zeroing only the untouched rows in that launch left partially
//     written lines behind for the touched rows to complete later: 95 us against 75 in the micro-benchmark.)
template <int LINE>
__global__ void __launch_bounds__(LG_REGION) k_zero_touched(const uint8_t* __restrict__ touched, float4* __restrict__ acc, size_t P,
                                                           uint8_t* __restrict__ tlist, uint16_t* __restrict__ tcount, const ZeroRows zr,
                                                           const uint32_t* __restrict__ det_mode, long long* __restrict__ acc64) {
    __shared__ uint32_t s_wcnt[LG_REGION / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t base = (size_t)blockIdx.x * LG_REGION;
    const size_t i = base + tid;
    const bool mark = i < P && touched[i] != 0;
    const unsigned long long m0 = __ballot(mark);
    if (lane == 0) s_wcnt[wv] = (uint32_t)__popcll(m0);
    {
        unsigned long long m = m0;
        const size_t wbase = i - (size_t)lane;
        constexpr int PER = 64 / LINE;                                 // lines cleared per store instruction
        const int sub = lane / LINE, part = lane % LINE;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        while (m) {
            // the next PER marked Gaussians of the wave: lane group `sub` takes the sub-th of them
            unsigned long long mm = m;
            int mine = -1;
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const int j = mm ? __builtin_ctzll(mm) : -1;
                if (k == sub) mine = j;
                mm &= mm - 1ull;
            }
            m = mm;
            if (mine >= 0) acc[(wbase + (size_t)mine) * LINE + part] = z;
        }
    }
    if (det_mode && (*det_mode & LG_MODE_DETERMINISTIC) != 0u && mark) {                         // deterministic buffers: the marked Gaussians' 128-byte fixed-point lines too
        float4* const w = reinterpret_cast<float4*>(acc64 + 16 * i);
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (i < P) {
        for (int k = 0; k < zr.n; k++) {                               // (wave-uniform: the pointers and widths are scalar loads from the arguments)
            float* q = zr.p[k];
            switch (zr.w[k]) {                                         // (uniform over the launch)
                case 1: q[i] = 0.f; break;
                case 2: put2(q, i, 0.f, 0.f); break;
                case 3: put3(q, i, 0.f, 0.f, 0.f); break;
                case 4: put4(q, i, 0.f, 0.f, 0.f, 0.f); break;
                case 6: put3(q, 2 * i, 0.f, 0.f, 0.f); put3(q, 2 * i + 1, 0.f, 0.f, 0.f); break;
                default: for (int c = 0; c < zr.w[k]; c += 3) put3(q, (size_t)(zr.w[k] / 3) * i + c / 3, 0.f, 0.f, 0.f); break;   // 9
            }
        }
    }
    __syncthreads();
    uint32_t off = 0, total = 0;
#pragma unroll
    for (int v = 0; v < LG_REGION / 64; v++) { off += v < wv ? s_wcnt[v] : 0u; total += s_wcnt[v]; }
    if (mark) tlist[base + off + (uint32_t)__popcll(m0 & ((1ull << lane) - 1ull))] = (uint8_t)tid;
    if (tid == 0) tcount[blockIdx.x] = (uint16_t)total;
}
void launch_zero_touched(const uint8_t* touched, float4* acc, int line_f4, size_t P, uint8_t* tlist, uint16_t* tcount, const ZeroRows& zr, hipStream_t s,
                         const uint32_t* det_mode, long long* acc64) {
    const unsigned blocks = (unsigned)((P + LG_REGION - 1) / LG_REGION);
    if (!blocks) return;
    if (line_f4 == 8) hipLaunchKernelGGL(k_zero_touched<8>, dim3(blocks), dim3(LG_REGION), 0, s, touched, acc, P, tlist, tcount, zr, det_mode, acc64);
    else hipLaunchKernelGGL(k_zero_touched<4>, dim3(blocks), dim3(LG_REGION), 0, s, touched, acc, P, tlist, tcount, zr, det_mode, acc64);
}
// the one-segment plan has no contribution flags: every VISIBLE Gaussian may be added to.  The culled ones stay unmarked -- their rows
// must be the exact zeros the reference's torch::zeros leaves (the chain on zero sums would turn a huge or non-finite scale into 0 * inf)
__global__ void __launch_bounds__(256) k_touch_visible(uint8_t* __restrict__ touched, const int* __restrict__ radii, size_t P) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < P) touched[i] = radii[i] > 0 ? 1 : 0;
}
void launch_touch_all(uint8_t* touched, const int* radii, size_t P, hipStream_t s) {
    hipLaunchKernelGGL(k_touch_visible, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, touched, radii, P);
}

void launch_gaussian_backward(const GaussBwdArgs& a, hipStream_t s) {
    const unsigned regions = (unsigned)((a.P + LG_REGION - 1) / LG_REGION);
    hipLaunchKernelGGL(k_gaussian_backward, dim3((regions + 3) / 4), dim3(256), 0, s, a);
}
// the pose form + the fold: a.view_partials holds 16 floats per region (view_partial_floats), dL_dviewmatrix 16 floats
void launch_gaussian_backward_view(const GaussBwdArgs& a, float* dL_dviewmatrix, hipStream_t s) {
    const unsigned regions = (unsigned)((a.P + LG_REGION - 1) / LG_REGION);
    hipLaunchKernelGGL(k_gaussian_backward_view, dim3((regions + 3) / 4), dim3(256), 0, s, a);
    launch_fold_view_partials(a.view_partials, (int)regions, dL_dviewmatrix, s);
}
void launch_fold_view_partials(const float* partials, int rows, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_fold_view_partials, dim3(1), dim3(16 * LG_VIEW_FOLD_GROUPS), 0, s, partials, rows, out);
}
size_t view_partial_floats(int P) { return P > 0 ? 16 * (((size_t)P + LG_REGION - 1) / LG_REGION) : 0; }

}  // namespace lg
