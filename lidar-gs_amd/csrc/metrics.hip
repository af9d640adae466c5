// metrics.hip -- the per-view evaluation of training_report on the device (include/lidargs_metrics.h; DESIGN.md section
// "Per-view evaluation").
//
//   k_vm_prepare   one grid-stride pass over the pixels (VM_PREP_BLOCKS fixed blocks): the image and the ground-truth intensity for
//                  the SSIM, depth_r / gt_depth for the points meter, the order-preserving keys of e and d for the medians, and one
//                  float64 partial per block of sum e, sum e*e, sum d, sum d*d (each thread in index order, then a fixed tree).
//                  Block 0 also clears the median histograms and the selection state.
//   (points meter) lidargs_points_meter on depth_r / gt_depth, unchanged, into a float32[6] of the scratch
//   k_vm_ssim      16 x 64 output tiles of the cropped SSIM map; the 22 x 70 input tile sits in LDS, every output sums its 7 x 7 window
//                  in float64 (x, y and the float32 products x*x, y*y, x*y), rounds the five means to float32 and evaluates S in float32
//                  as scikit-image writes it; one float64 partial per block
//   k_vm_hist      x 3   radix select, digits of 11, 11 and 10 bits from the top: a 2048-bin histogram per array in LDS (integer
//                        atomics), added to the global one; only keys whose higher digits match the prefix chosen so far are counted
//   k_vm_pick      x 2   one workgroup: per array, the bin that holds rank (n-1)/2, the rank within it, the longer prefix; clears the
//                        histograms for the next pass
//   k_vm_finish    one workgroup: the last pick, every partial folded in a fixed order, the 11 outputs
// Eight launches plus the points meter's; no host read, no float atomics.  Built with -ffp-contract=off: S and the means round as
// written.
#include "lidargs_common.h"
#include "../../include/lidargs_rasterizer.h"
#include "../../include/lidargs_chamfer.h"
#include "../../include/lidargs_metrics.h"
#include <math.h>
#include <stdint.h>

namespace lg {

#define VM_THREADS 256
#define VM_PREP_BLOCKS 256
#define VM_HIST_BLOCKS 256
#define VM_BINS 2048
#define VM_TX 64                    // SSIM output tile: columns
#define VM_TY 16                    //                   rows
#define VM_HALO 3

struct VmWork {
    char* pm;                       // the points meter's scratch
    float *img, *gti, *depth_r, *gt_depth, *pm_out;
    uint32_t *key_e, *key_d, *hist, *state;
    double *part, *ssim_part;
    int ssim_blocks;
};

static int vm_ssim_gx(int W) { return (W - 2 * VM_HALO + VM_TX - 1) / VM_TX; }
static int vm_ssim_gy(int H) { return (H - 2 * VM_HALO + VM_TY - 1) / VM_TY; }

static size_t vm_carve(char* base, int H, int W, int with_pm, VmWork* w) {
    Carver c(base);
    VmWork k;
    const size_t n = (size_t)H * W;
    const size_t pm_bytes = with_pm ? lidargs_points_meter_scratch_bytes(H, W) : 0;
    k.pm = c.take<char>(pm_bytes);
    k.img = c.take<float>(n); k.gti = c.take<float>(n); k.depth_r = c.take<float>(n); k.gt_depth = c.take<float>(n);
    k.key_e = c.take<uint32_t>(n); k.key_d = c.take<uint32_t>(n);
    k.part = c.take<double>(4 * VM_PREP_BLOCKS);
    k.ssim_blocks = vm_ssim_gx(W) * vm_ssim_gy(H);
    k.ssim_part = c.take<double>(k.ssim_blocks);
    k.hist = c.take<uint32_t>(2 * VM_BINS); k.state = c.take<uint32_t>(4); k.pm_out = c.take<float>(8);
    if (w) *w = k;
    return (size_t)(c.p - base) + 128;
}

// torch.clamp: NaN passes through (fminf / fmaxf would drop it)
__device__ __forceinline__ float clamp_t(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

// the order-preserving image of a float as an unsigned key (negative values flipped, positive ones above them; NaN above +inf)
__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// fixed-order block sum of VM_THREADS doubles: the same tree every call
__device__ double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = VM_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(VM_THREADS) k_vm_prepare(int n, const float* __restrict__ render, const float* __restrict__ depth,
                                                           const float* __restrict__ gt, float dmin, float dmax, VmWork w) {
    __shared__ double sh[VM_THREADS];
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        for (int i = t; i < 2 * VM_BINS; i += VM_THREADS) w.hist[i] = 0u;
        if (t < 4) w.state[t] = 0u;     // (prefix, rank) per array; the first pick sets the ranks
    }
    double se = 0.0, see = 0.0, sd = 0.0, sdd = 0.0;
    for (int i = blockIdx.x * VM_THREADS + t; i < n; i += VM_PREP_BLOCKS * VM_THREADS) {
        const float rd = render[n + i];
        const float mask = rd > 0.5f ? 1.0f : 0.0f;                          // torch.where(render_raydrop > 0.5, 1, 0), promoted
        const float img = clamp_t(render[i], 0.0f, 1.0f) * mask;
        const float g0 = gt[i];
        const float gti = gt[n + i] * g0;
        const float e = fabsf(img - gti);
        const float dr = clamp_t(depth[i], dmin, dmax) * mask;
        const float gd = gt[2 * n + i] * g0;
        const float d = fabsf(dr - gd);
        w.img[i] = img; w.gti[i] = gti; w.depth_r[i] = dr; w.gt_depth[i] = gd;
        w.key_e[i] = f2key(e); w.key_d[i] = f2key(d);
        const float ee = e * e, dd = d * d;
        se += (double)e; see += (double)ee; sd += (double)d; sdd += (double)dd;
    }
    se = block_sum(se, sh); see = block_sum(see, sh); sd = block_sum(sd, sh); sdd = block_sum(sdd, sh);
    if (t == 0) {
        w.part[blockIdx.x] = se; w.part[VM_PREP_BLOCKS + blockIdx.x] = see;
        w.part[2 * VM_PREP_BLOCKS + blockIdx.x] = sd; w.part[3 * VM_PREP_BLOCKS + blockIdx.x] = sdd;
    }
}

__global__ void __launch_bounds__(VM_THREADS) k_vm_ssim(int H, int W, const float* __restrict__ X, const float* __restrict__ Y,
                                                        double* __restrict__ part) {
    constexpr int LW = VM_TX + 2 * VM_HALO, LH = VM_TY + 2 * VM_HALO;
    __shared__ float sx[LH][LW + 1];
    __shared__ float sy[LH][LW + 1];
    __shared__ double sh[VM_THREADS];
    const int t = threadIdx.x;
    const int c0 = VM_HALO + blockIdx.x * VM_TX, r0 = VM_HALO + blockIdx.y * VM_TY;      // first output pixel of the tile
    for (int k = t; k < LH * LW; k += VM_THREADS) {
        const int rr = k / LW, cc = k % LW;
        const int gr = r0 - VM_HALO + rr, gc = c0 - VM_HALO + cc;                       // >= 0 always
        const bool in = gr < H && gc < W;
        sx[rr][cc] = in ? X[(size_t)gr * W + gc] : 0.0f;
        sy[rr][cc] = in ? Y[(size_t)gr * W + gc] : 0.0f;
    }
    __syncthreads();
    const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);        // (K * data_range)^2 in double, then float32 as numpy does
    const float cov_norm = (float)(49.0 / 48.0);
    const int oc = t % VM_TX;
    double acc = 0.0;
    for (int orow = t / VM_TX; orow < VM_TY; orow += VM_THREADS / VM_TX) {
        const int r = r0 + orow, c = c0 + oc;
        if (r >= H - VM_HALO || c >= W - VM_HALO) continue;
        double s1 = 0.0, s2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
        for (int dy = 0; dy < 7; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) {
                const float x = sx[orow + dy][oc + dx], y = sy[orow + dy][oc + dx];
                const float xx = x * x, yy = y * y, xy = x * y;
                s1 += (double)x; s2 += (double)y; s11 += (double)xx; s22 += (double)yy; s12 += (double)xy;
            }
        }
        const float ux = (float)(s1 / 49.0), uy = (float)(s2 / 49.0);
        const float uxx = (float)(s11 / 49.0), uyy = (float)(s22 / 49.0), uxy = (float)(s12 / 49.0);
        const float vx = cov_norm * (uxx - ux * ux);
        const float vy = cov_norm * (uyy - uy * uy);
        const float vxy = cov_norm * (uxy - ux * uy);
        const float A1 = 2.0f * ux * uy + C1, A2 = 2.0f * vxy + C2;
        const float B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
        const float D = B1 * B2;
        const float S = (A1 * A2) / D;
        acc += (double)S;
    }
    acc = block_sum(acc, sh);
    if (t == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

struct VmPass { int shift, bits; };
__device__ __forceinline__ VmPass vm_pass(int p) { return p == 0 ? VmPass{21, 11} : p == 1 ? VmPass{10, 11} : VmPass{0, 10}; }

__global__ void __launch_bounds__(VM_THREADS) k_vm_hist(int n, int pass, const uint32_t* __restrict__ key_e, const uint32_t* __restrict__ key_d,
                                                        uint32_t* __restrict__ hist, const uint32_t* __restrict__ state) {
    __shared__ uint32_t h[2 * VM_BINS];
    const int t = threadIdx.x;
    for (int i = t; i < 2 * VM_BINS; i += VM_THREADS) h[i] = 0u;
    __syncthreads();
    const VmPass P = vm_pass(pass);
    const int hi = P.shift + P.bits;                      // the bits above this digit were chosen by the earlier passes
    const uint32_t mask = (1u << P.bits) - 1u;
    const uint32_t pe = state[0], pd = state[2];
    for (int i = blockIdx.x * VM_THREADS + t; i < n; i += gridDim.x * VM_THREADS) {
        const uint32_t ke = key_e[i], kd = key_d[i];
        if (hi >= 32 || (ke >> hi) == pe) atomicAdd(&h[(ke >> P.shift) & mask], 1u);
        if (hi >= 32 || (kd >> hi) == pd) atomicAdd(&h[VM_BINS + ((kd >> P.shift) & mask)], 1u);
    }
    __syncthreads();
    for (int i = t; i < 2 * VM_BINS; i += VM_THREADS)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// One workgroup: for both arrays, the bin of this pass's digit that holds the wanted rank.  state = (prefix_e, rank_e, prefix_d, rank_d);
// pass 0 starts from rank (n-1)/2.  Clears the histogram for the next pass.
__device__ void vm_pick(int n, int pass, uint32_t* hist, uint32_t* state) {
    __shared__ uint32_t scan[VM_THREADS];
    constexpr int PER = VM_BINS / VM_THREADS;               // 8 bins per thread
    const int t = threadIdx.x;
    const VmPass P = vm_pass(pass);
    const int nb = 1 << P.bits;
    for (int a = 0; a < 2; ++a) {
        const uint32_t* hb = hist + a * VM_BINS;
        const uint32_t rank = pass == 0 ? (uint32_t)((n - 1) / 2) : state[2 * a + 1];
        const uint32_t prefix = pass == 0 ? 0u : state[2 * a];
        uint32_t mine = 0;
        for (int j = 0; j < PER; ++j) {
            const int b = t * PER + j;
            mine += b < nb ? hb[b] : 0u;
        }
        scan[t] = mine;
        __syncthreads();
        for (int s = 1; s < VM_THREADS; s <<= 1) {          // inclusive Hillis-Steele scan
            const uint32_t v = t >= s ? scan[t - s] : 0u;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        const uint32_t incl = scan[t], excl = incl - mine;
        if (excl <= rank && rank < incl) {                  // exactly one thread: the counts of this pass add up to more than rank
            uint32_t cum = excl;
            for (int j = 0; j < PER; ++j) {
                const int b = t * PER + j;
                const uint32_t c = b < nb ? hb[b] : 0u;
                if (rank < cum + c) {
                    state[2 * a] = (prefix << P.bits) | (uint32_t)b;
                    state[2 * a + 1] = rank - cum;
                    break;
                }
                cum += c;
            }
        }
        __syncthreads();
    }
    for (int i = t; i < 2 * VM_BINS; i += VM_THREADS) hist[i] = 0u;
    __syncthreads();
}

__global__ void __launch_bounds__(VM_THREADS) k_vm_pick(int n, int pass, uint32_t* hist, uint32_t* state) { vm_pick(n, pass, hist, state); }

__global__ void __launch_bounds__(VM_THREADS) k_vm_finish(int H, int W, int with_pm, VmWork w, double* __restrict__ out) {
    __shared__ double sh[VM_THREADS];
    const int n = H * W;
    const int t = threadIdx.x;
    vm_pick(n, 2, w.hist, w.state);
    double q[4];
    for (int k = 0; k < 4; ++k) q[k] = block_sum(w.part[k * VM_PREP_BLOCKS + t], sh);        // VM_PREP_BLOCKS == VM_THREADS
    double s = 0.0;
    for (int i = t; i < w.ssim_blocks; i += VM_THREADS) s += w.ssim_part[i];
    s = block_sum(s, sh);
    if (t != 0) return;
    const double nn = (double)n;
    const float me = (float)(q[0] / nn), mse = (float)(q[1] / nn), md = (float)(q[2] / nn), msd = (float)(q[3] / nn);
    const float psnr = 20.0f * log10f(1.0f / sqrtf(mse));
    const double qnan = __builtin_nan("");
    out[0] = (double)me;
    out[1] = (double)psnr;
    out[2] = s / ((double)(H - 2 * VM_HALO) * (double)(W - 2 * VM_HALO));
    out[3] = (double)me;
    out[4] = (double)sqrtf(mse);
    out[5] = q[0] != q[0] ? qnan : (double)key2f(w.state[0]);       // a NaN error makes the sum NaN (every e >= 0 or NaN)
    out[6] = with_pm ? (double)w.pm_out[0] : qnan;
    out[7] = with_pm ? (double)w.pm_out[1] : qnan;
    out[8] = (double)md;
    out[9] = q[2] != q[2] ? qnan : (double)key2f(w.state[2]);
    out[10] = (double)sqrtf(msd);
}

}  // namespace lg

extern "C" {

size_t lidargs_view_metrics_scratch_bytes(int H, int W) {
    if (H < 7 || W < 7 || (long long)H * W > (1ll << 28)) return 0;
    return lg::vm_carve(nullptr, H, W, 1, nullptr);
}

int lidargs_view_metrics_ex(int H, int W, const float* render, const float* depth, const float* gt, float depth_min, float depth_max,
                            const float* beam_inclinations, float fov_up, float fov, int with_points_meter, double* out, char* scratch,
                            size_t scratch_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (H < 7 || W < 7) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "view_metrics: the SSIM window (7 x 7) needs H >= 7 and W >= 7");
    if ((long long)H * W > (1ll << 28)) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "view_metrics: image too large (H * W > 2^28)");
    if (!render || !depth || !gt || !out || !scratch) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "view_metrics: NULL pointer");
    const int with_pm = with_points_meter ? 1 : 0;
    if (scratch_bytes < lg::vm_carve(nullptr, H, W, with_pm, nullptr)) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "view_metrics: scratch too small");
    const int n = H * W;
    lg::VmWork w;
    lg::vm_carve(scratch, H, W, with_pm, &w);
    hipLaunchKernelGGL(lg::k_vm_prepare, dim3(VM_PREP_BLOCKS), dim3(VM_THREADS), 0, stream, n, render, depth, gt, depth_min, depth_max, w);
    if (with_pm) {
        const int rc = lidargs_points_meter(H, W, w.depth_r, w.gt_depth, 1.0f, beam_inclinations, fov_up, fov, 0.05f, w.pm_out, w.pm,
                                            lidargs_points_meter_scratch_bytes(H, W), stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(lg::k_vm_ssim, dim3(lg::vm_ssim_gx(W), lg::vm_ssim_gy(H)), dim3(VM_THREADS), 0, stream, H, W, w.img, w.gti, w.ssim_part);
    const int hb = n < VM_HIST_BLOCKS * VM_THREADS ? (n + VM_THREADS - 1) / VM_THREADS : VM_HIST_BLOCKS;
    for (int pass = 0; pass < 3; ++pass) {
        hipLaunchKernelGGL(lg::k_vm_hist, dim3(hb), dim3(VM_THREADS), 0, stream, n, pass, w.key_e, w.key_d, w.hist, w.state);
        if (pass < 2) hipLaunchKernelGGL(lg::k_vm_pick, dim3(1), dim3(VM_THREADS), 0, stream, n, pass, w.hist, w.state);
    }
    hipLaunchKernelGGL(lg::k_vm_finish, dim3(1), dim3(VM_THREADS), 0, stream, H, W, with_pm, w, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lg::api_fail(LIDARGS_ERR_HIP, hipGetErrorString(e));
    return 0;
}

int lidargs_view_metrics(int H, int W, const float* render, const float* depth, const float* gt, float depth_min, float depth_max,
                         const float* beam_inclinations, float fov_up, float fov, double* out, char* scratch, size_t scratch_bytes,
                         void* stream) {
    return lidargs_view_metrics_ex(H, W, render, depth, gt, depth_min, depth_max, beam_inclinations, fov_up, fov, 1, out, scratch,
                                   scratch_bytes, stream);
}

}  // extern "C"
