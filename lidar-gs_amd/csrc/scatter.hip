// scatter.hip -- scatter_max / scatter_min with the winning position, and their gradient (include_scatter/lidargs_scatter.h, which
// states the semantics; DESIGN.md section "Scatter max / min").  The only source of liblidargs_scatter.so.
//
// src is [A, E, B]; element i = (a * E + e) * B + b reduces into output slot (a * G + index(a, e, b)) * B + b.  One 64-bit key per slot:
//     key = ordered(value) << 32 | position code
//   ordered()      the order-preserving image of float bits in u32: negative floats ~bits, the others bits | 0x80000000; so
//                  -inf = 0x007fffff < ... < -0.0 = 0x7fffffff < +0.0 = 0x80000000 < ... < +inf = 0xff800000.  0 and 0xffffffff are images
//                  of no number: the winning one of the two (max: 0xffffffff, min: 0) is what EVERY NaN maps to, the other is the identity.
//   position code  max: kept = 0xffffffff, element e = 0xfffffffe - e;  min: kept = 0, element e = e + 1  (E < 2^31).  Among equal values
//                  atomicMax / atomicMin then leaves the kept initial value before any element, and the lowest e among elements.
// forward, three launches:
//   k_sc_fill     every key = the identity, or the key of out's initial value; both with the kept code
//   k_sc_reduce   one lane per element, grid-stride, consecutive lanes consecutive b: with a broadcast index a wave's 64
//                 atomics go to 64 different keys of the same few lines.  A key only ever moves one way, so an element that does not beat what
//                 a relaxed load sees cannot win and issues no atomic (as k_rv_project of range_view.hip).  An index value outside [0, G) is skipped.
//   k_sc_resolve  one lane per slot: key -> out, arg.  Every slot is written here, so nothing is zero-filled first.
// backward, one launch (k_sc_backward): one lane per element of src; no atomic, no zero-fill.
// The divisions that split i into (a, e, b) are 32-bit whenever every count fits (Idx = unsigned), 64-bit otherwise.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include_scatter/lidargs_scatter.h"
#include "lidargs_status.h"

namespace {

typedef unsigned long long u64;

constexpr int SC_THREADS = 256;
constexpr long long SC_MAX_BLOCKS = 2048;                  // 256 CUs x 8 workgroups (8 waves a SIMD); beyond 524 288 lanes, grid-stride rounds
constexpr size_t SC_MAX_E = (size_t)1 << 31;
constexpr size_t SC_MAX_COUNT = (size_t)1 << 60;           // of elements of src or out: leaves room for the byte counts
constexpr unsigned SC_QUIET_NAN = 0x7fc00000u;

template <int OP> struct Key;
template <> struct Key<LIDARGS_SCATTER_MAX> {
    static constexpr unsigned NAN_IMAGE = 0xffffffffu, IDENTITY = 0u, KEPT = 0xffffffffu;
    static __device__ __forceinline__ unsigned code(unsigned e) { return 0xfffffffeu - e; }
    static __device__ __forceinline__ unsigned position(unsigned code) { return 0xfffffffeu - code; }
    static __device__ __forceinline__ void merge(u64* slot, u64 key) {
        if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(slot, key);
    }
};
template <> struct Key<LIDARGS_SCATTER_MIN> {
    static constexpr unsigned NAN_IMAGE = 0u, IDENTITY = 0xffffffffu, KEPT = 0u;
    static __device__ __forceinline__ unsigned code(unsigned e) { return e + 1u; }
    static __device__ __forceinline__ unsigned position(unsigned code) { return code - 1u; }
    static __device__ __forceinline__ void merge(u64* slot, u64 key) {
        if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(slot, key);
    }
};

template <int OP> __device__ __forceinline__ unsigned ordered(float v) {
    if (v != v) return Key<OP>::NAN_IMAGE;
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int OP> __device__ __forceinline__ float value_of(unsigned image) {
    if (image == Key<OP>::NAN_IMAGE) return __uint_as_float(SC_QUIET_NAN);
    return __uint_as_float((image & 0x80000000u) ? (image ^ 0x80000000u) : ~image);
}

__device__ __forceinline__ u64 make_key(unsigned image, unsigned code) { return ((u64)image << 32) | code; }

// the shape of src and of the index, as the kernels need it
struct Shape { size_t E, B, G, sa, se, sb; };

// element i of src -> its position e and its output slot; false when its index value is outside [0, G)
template <typename Idx>
__device__ __forceinline__ bool locate(const Shape& s, const long long* __restrict__ index, size_t i, unsigned& e, size_t& slot) {
    const Idx r = (Idx)i / (Idx)s.B, b = (Idx)i - r * (Idx)s.B;
    const Idx a = r / (Idx)s.E;
    e = (unsigned)(r - a * (Idx)s.E);
    const long long g = index[(size_t)a * s.sa + (size_t)e * s.se + (size_t)b * s.sb];
    if ((u64)g >= (u64)s.G) return false;                  // (a negative value is a huge unsigned one)
    slot = ((size_t)a * s.G + (size_t)g) * s.B + (size_t)b;
    return true;
}

template <int OP>
__global__ void __launch_bounds__(SC_THREADS) k_sc_fill(size_t n_out, const float* __restrict__ initial, u64* __restrict__ keys) {
    const size_t stride = (size_t)gridDim.x * SC_THREADS;
    for (size_t i = (size_t)blockIdx.x * SC_THREADS + threadIdx.x; i < n_out; i += stride)
        keys[i] = make_key(initial ? ordered<OP>(initial[i]) : Key<OP>::IDENTITY, Key<OP>::KEPT);
}

template <int OP, typename Idx>
__global__ void __launch_bounds__(SC_THREADS) k_sc_reduce(size_t n, Shape s, const float* __restrict__ src, const long long* __restrict__ index,
                                                          u64* keys) {
    const size_t stride = (size_t)gridDim.x * SC_THREADS;
    for (size_t i = (size_t)blockIdx.x * SC_THREADS + threadIdx.x; i < n; i += stride) {
        unsigned e;
        size_t slot;
        if (!locate<Idx>(s, index, i, e, slot)) continue;
        Key<OP>::merge(keys + slot, make_key(ordered<OP>(src[i]), Key<OP>::code(e)));
    }
}

template <int OP>
__global__ void __launch_bounds__(SC_THREADS) k_sc_resolve(size_t n_out, long long E, int use_initial, const u64* __restrict__ keys,
                                                           float* __restrict__ out, long long* __restrict__ arg) {
    const size_t stride = (size_t)gridDim.x * SC_THREADS;
    for (size_t i = (size_t)blockIdx.x * SC_THREADS + threadIdx.x; i < n_out; i += stride) {
        const u64 k = keys[i];
        const unsigned image = (unsigned)(k >> 32), code = (unsigned)k;
        if (code == Key<OP>::KEPT) {                       // no element won: an empty group, or an initial value that stays as it is
            arg[i] = E;
            if (!use_initial) out[i] = 0.0f;
        } else {
            arg[i] = (long long)Key<OP>::position(code);
            out[i] = value_of<OP>(image);
        }
    }
}

template <typename Idx>
__global__ void __launch_bounds__(SC_THREADS) k_sc_backward(size_t n, Shape s, const long long* __restrict__ index, const long long* __restrict__ arg,
                                                            const float* __restrict__ grad_out, float* __restrict__ grad_src) {
    const size_t stride = (size_t)gridDim.x * SC_THREADS;
    for (size_t i = (size_t)blockIdx.x * SC_THREADS + threadIdx.x; i < n; i += stride) {
        unsigned e;
        size_t slot;
        float g = 0.0f;
        if (locate<Idx>(s, index, i, e, slot) && arg[slot] == (long long)e) g = grad_out[slot];
        grad_src[i] = g;
    }
}

int grid_for(size_t n) {
    const size_t blocks = (n + SC_THREADS - 1) / SC_THREADS;
    return (int)(blocks < (size_t)SC_MAX_BLOCKS ? blocks : (size_t)SC_MAX_BLOCKS);
}

// a * b * c into *out; false when it does not fit SC_MAX_COUNT
bool product(size_t a, size_t b, size_t c, size_t* out) {
    size_t ab;
    if (__builtin_mul_overflow(a, b, &ab) || __builtin_mul_overflow(ab, c, out)) return false;
    return *out <= SC_MAX_COUNT;
}

// 0, or what is wrong with the sizes; n = A * E * B, n_out = A * G * B
const char* check_sizes(size_t A, size_t E, size_t B, size_t G, size_t* n, size_t* n_out) {
    if (E >= SC_MAX_E) return "E must be below 2^31 (the position shares the key with the value)";
    if (!product(A, E, B, n) || !product(A, G, B, n_out)) return "A * E * B or A * G * B does not fit";
    return nullptr;
}

// whether 32-bit arithmetic splits every i < n into (a, e, b)
bool narrow(size_t n) { return n <= 0xffffffffull; }

template <int OP>
void forward(size_t n, size_t n_out, const Shape& s, const float* src, const long long* index, int use_initial, float* out, long long* arg,
             u64* keys, hipStream_t stream) {
    hipLaunchKernelGGL(k_sc_fill<OP>, dim3(grid_for(n_out)), dim3(SC_THREADS), 0, stream, n_out, use_initial ? out : nullptr, keys);
    if (n > 0) {
        if (narrow(n)) hipLaunchKernelGGL((k_sc_reduce<OP, unsigned>), dim3(grid_for(n)), dim3(SC_THREADS), 0, stream, n, s, src, index, keys);
        else hipLaunchKernelGGL((k_sc_reduce<OP, u64>), dim3(grid_for(n)), dim3(SC_THREADS), 0, stream, n, s, src, index, keys);
    }
    hipLaunchKernelGGL(k_sc_resolve<OP>, dim3(grid_for(n_out)), dim3(SC_THREADS), 0, stream, n_out, (long long)s.E, use_initial, keys, out, arg);
}

}  // namespace

extern "C" {

int lidargs_scatter_abi_version(void) { return LIDARGS_SCATTER_ABI_VERSION; }
const char* lidargs_scatter_last_error(void) { return g_err; }

size_t lidargs_scatter_scratch_bytes(size_t n_out) { return n_out <= SC_MAX_COUNT ? n_out * sizeof(u64) : 0; }

int lidargs_scatter_extreme(int op, size_t A, size_t E, size_t B, size_t G, const float* src, const long long* index,
                            size_t sa, size_t se, size_t sb, int use_initial, float* out, long long* arg,
                            char* scratch, size_t scratch_bytes, void* stream) {
    const char* what = "scatter_extreme";
    size_t n, n_out;
    if (op != LIDARGS_SCATTER_MAX && op != LIDARGS_SCATTER_MIN) return fail(-1, what, "unknown op (0 = max, 1 = min)");
    if (use_initial != 0 && use_initial != 1) return fail(-1, what, "use_initial must be 0 or 1");
    if (const char* m = check_sizes(A, E, B, G, &n, &n_out)) return fail(-1, what, m);
    if (n_out == 0) return 0;
    if ((n > 0 && (!src || !index)) || !out || !arg || !scratch) return fail(-1, what, "NULL pointer");
    if (scratch_bytes < lidargs_scatter_scratch_bytes(n_out) || ((uintptr_t)scratch & 7)) return fail(-1, what, "scratch too small or not 8-byte aligned");
    const Shape s{E, B, G, sa, se, sb};
    u64* keys = reinterpret_cast<u64*>(scratch);
    if (op == LIDARGS_SCATTER_MAX) forward<LIDARGS_SCATTER_MAX>(n, n_out, s, src, index, use_initial, out, arg, keys, (hipStream_t)stream);
    else forward<LIDARGS_SCATTER_MIN>(n, n_out, s, src, index, use_initial, out, arg, keys, (hipStream_t)stream);
    return launched(-4, what);
}

int lidargs_scatter_extreme_backward(size_t A, size_t E, size_t B, size_t G, const long long* index, size_t sa, size_t se, size_t sb,
                                     const long long* arg, const float* grad_out, float* grad_src, void* stream) {
    const char* what = "scatter_extreme_backward";
    size_t n, n_out;
    if (const char* m = check_sizes(A, E, B, G, &n, &n_out)) return fail(-1, what, m);
    if (n == 0) return 0;
    if (!index || !grad_src || (n_out > 0 && (!arg || !grad_out))) return fail(-1, what, "NULL pointer");
    const Shape s{E, B, G, sa, se, sb};
    if (narrow(n)) hipLaunchKernelGGL(k_sc_backward<unsigned>, dim3(grid_for(n)), dim3(SC_THREADS), 0, (hipStream_t)stream, n, s, index, arg, grad_out, grad_src);
    else hipLaunchKernelGGL(k_sc_backward<u64>, dim3(grid_for(n)), dim3(SC_THREADS), 0, (hipStream_t)stream, n, s, index, arg, grad_out, grad_src);
    return launched(-4, what);
}

}  // extern "C"
