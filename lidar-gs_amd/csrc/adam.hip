// adam.hip -- the optimizer step of the whole model in one launch (include_optim/lidargs_optim.h; DESIGN.md section "Optimizer step").
// The only source of liblidargs_optim.so: nothing here is linked into liblidargs_hip.so.
//
//   k_adam   one workgroup of 256 threads per chunk of ADAM_CHUNK consecutive elements of ONE tensor.  The table of tensors and the
//            running chunk counts sit in the kernel argument (3.4 KB): a workgroup finds its tensor by counting the prefix entries its
//            index has passed -- scalar loads and scalar compares, the same in every lane.  Inside the chunk every thread issues the
//            dwordx4 loads of its four float4s of each of the four streams (param, grad, exp_avg, exp_avg_sq) before the first use,
//            and stores three.  The last n % 4 elements of a tensor, and every element of a tensor whose four pointers are not all
//            16-byte aligned (the flag is taken on the host), go through 4-byte accesses.
// 28 bytes per element (four loads, three stores), ~12 float operations: HBM-bound.
// Built with -ffp-contract=off: every operation rounds as written, and the three fused steps torch's device kernels make are written
// as fmaf.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include_optim/lidargs_optim.h"
#include "lidargs_status.h"

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_CHUNK = 4096;                       // elements per workgroup: 4 float4 per thread and stream
constexpr int ADAM_VEC_ROUNDS = ADAM_CHUNK / (4 * ADAM_THREADS);

struct AdamArgs {
    lidargs_adam_tensor t[LIDARGS_ADAM_MAX_TENSORS];
    uint32_t chunk_end[LIDARGS_ADAM_MAX_TENSORS];      // chunks of tensors 0..i; 0xFFFFFFFF behind the last tensor
    uint64_t aligned;                                  // bit i: the four pointers of tensor i are 16-byte aligned
    float w1, one_minus_w1, b2, w2, eps;
};
static_assert(sizeof(AdamArgs) <= 4096, "the table must fit the kernel argument segment");

struct Coef { float w1, one_minus_w1, b2, w2, eps, inv_bc2_sqrt, neg_step; };

// One element, operation by operation as torch's device kernels evaluate _single_tensor_adam (lerp_, mul_, addcmul_, sqrt, div by a
// Python scalar = multiplication by the float32 reciprocal, add_, addcdiv_).
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const Coef& c) {
    const float d = g - m;
    m = c.w1 < 0.5f ? fmaf(c.w1, d, m) : fmaf(-d, c.one_minus_w1, g);
    v = fmaf(c.w2, g * g, v * c.b2);
    const float denom = sqrtf(v) * c.inv_bc2_sqrt + c.eps;
    p = fmaf(c.neg_step, m / denom, p);
}

__global__ __launch_bounds__(ADAM_THREADS) void k_adam(const AdamArgs a) {
    const uint32_t b = blockIdx.x;
    int ti = 0;
#pragma unroll
    for (int i = 0; i < LIDARGS_ADAM_MAX_TENSORS; i++) ti += (b >= a.chunk_end[i]) ? 1 : 0;
    const uint32_t first = ti ? a.chunk_end[ti - 1] : 0u;
    const lidargs_adam_tensor t = a.t[ti];
    const long long n = t.n;
    const long long lo = (long long)(b - first) * ADAM_CHUNK;
    const long long hi = lo + ADAM_CHUNK < n ? lo + ADAM_CHUNK : n;
    const Coef c = {a.w1, a.one_minus_w1, a.b2, a.w2, a.eps, t.inv_bias_correction2_sqrt, t.neg_step_size};
    float* __restrict__ P = t.param;
    const float* __restrict__ G = t.grad;
    float* __restrict__ M = t.exp_avg;
    float* __restrict__ V = t.exp_avg_sq;
    const int tid = threadIdx.x;

    if (!((a.aligned >> ti) & 1ull)) {                 // wave-uniform
        for (long long i = lo + tid; i < hi; i += ADAM_THREADS) {
            float p = P[i], m = M[i], v = V[i];
            adam_one(p, G[i], m, v, c);
            P[i] = p; M[i] = m; V[i] = v;
        }
        return;
    }
    const long long n4 = n & ~3ll;                     // the elements whole float4s cover
    const long long vhi = hi < n4 ? hi : n4;
    float4 p[ADAM_VEC_ROUNDS], g[ADAM_VEC_ROUNDS], m[ADAM_VEC_ROUNDS], v[ADAM_VEC_ROUNDS];
#pragma unroll
    for (int r = 0; r < ADAM_VEC_ROUNDS; r++) {
        const long long i = lo + (long long)(r * ADAM_THREADS + tid) * 4;
        if (i < vhi) {
            p[r] = *reinterpret_cast<const float4*>(P + i); g[r] = *reinterpret_cast<const float4*>(G + i);
            m[r] = *reinterpret_cast<const float4*>(M + i); v[r] = *reinterpret_cast<const float4*>(V + i);
        }
    }
#pragma unroll
    for (int r = 0; r < ADAM_VEC_ROUNDS; r++) {
        const long long i = lo + (long long)(r * ADAM_THREADS + tid) * 4;
        if (i < vhi) {
            adam_one(p[r].x, g[r].x, m[r].x, v[r].x, c); adam_one(p[r].y, g[r].y, m[r].y, v[r].y, c);
            adam_one(p[r].z, g[r].z, m[r].z, v[r].z, c); adam_one(p[r].w, g[r].w, m[r].w, v[r].w, c);
            *reinterpret_cast<float4*>(P + i) = p[r]; *reinterpret_cast<float4*>(M + i) = m[r]; *reinterpret_cast<float4*>(V + i) = v[r];
        }
    }
    const long long i = (lo > n4 ? lo : n4) + tid;     // the tail: at most 3 elements, in the tensor's last chunk
    if (i < hi) {
        float ps = P[i], ms = M[i], vs = V[i];
        adam_one(ps, G[i], ms, vs, c);
        P[i] = ps; M[i] = ms; V[i] = vs;
    }
}

}  // namespace

extern "C" {

int lidargs_adam_max_tensors(void) { return LIDARGS_ADAM_MAX_TENSORS; }
int lidargs_optim_abi_version(void) { return LIDARGS_OPTIM_ABI_VERSION; }
const char* lidargs_optim_last_error(void) { return g_err; }

int lidargs_adam_step(int n_tensors, const lidargs_adam_tensor* table, double beta1, double beta2, double eps, void* stream) {
    const char* what = "adam_step";
    if (n_tensors < 0 || n_tensors > LIDARGS_ADAM_MAX_TENSORS) return fail(-1, what, "n_tensors out of range");
    if (n_tensors > 0 && !table) return fail(-1, what, "NULL table");
    AdamArgs a;
    uint64_t chunks = 0;
    a.aligned = 0;
    for (int i = 0; i < LIDARGS_ADAM_MAX_TENSORS; i++) {
        if (i >= n_tensors) { a.t[i] = lidargs_adam_tensor{nullptr, nullptr, nullptr, nullptr, 0, 0.f, 0.f}; a.chunk_end[i] = 0xFFFFFFFFu; continue; }
        const lidargs_adam_tensor& t = table[i];
        if (t.n < 0) return fail(-1, what, "negative size");
        if (t.n > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) return fail(-1, what, "NULL pointer with n > 0");
        chunks += ((uint64_t)t.n + ADAM_CHUNK - 1) / ADAM_CHUNK;
        if (chunks > 0x7FFFFFFFull) return fail(-1, what, "too many elements for one call");
        a.t[i] = t;
        a.chunk_end[i] = (uint32_t)chunks;
        const uintptr_t bits = (uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq;
        if (!(bits & 15)) a.aligned |= 1ull << i;
    }
    if (chunks == 0) return 0;
    a.w1 = (float)(1.0 - beta1);
    a.one_minus_w1 = 1.0f - a.w1;
    a.b2 = (float)beta2;
    a.w2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    hipLaunchKernelGGL(k_adam, dim3((unsigned)chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, a);
    return launched(-4, what);
}

}  // extern "C"
