// knn.hip -- model initialisation of GaussianModel.create_from_pcd (include/lidargs_knn.h; DESIGN.md section "simple_knn drop-in").
//
// 1. lidargs_knn_mean_dist: the mean squared distance to the 3 nearest neighbours of every point (distCUDA2 of the third-party
//    simple_knn extension).  The contract (header) is exact: the result is a function of the multiset of the 3 smallest float32
//    squared distances, so the search below may skip only points that cannot enter that multiset.
//      k_knn_center   mean of the finite points (double atomics; it only steers the ORDER of the points, never a result)
//      k_knn_keys     63-bit Morton key of every finite point, from the top 21 bits of the order-preserving image of the float
//                     x - center per axis (sign, exponent, 12 mantissa bits: cells of relative size 2^-12 of the distance to the
//                     center, so a cloud whose density falls like 1/r^2 with outliers at 1e6 m still gets small cells where it is
//                     dense); non-finite points get the all-ones key and sort behind every finite one
//      sort           LSD radix on the low and the high word (binning.hip's pair sort, value = input row)
//      k_knn_leaves   the points in key order as float4 + the bounding box of every leaf of KNN_FAN consecutive points (finite only)
//      k_knn_parents  each upper level: the box of KNN_FAN consecutive children, until one level has at most KNN_FAN nodes
//      k_knn_query    one lane per point in key order: seed the 3 best from the query's own leaf, then one stackless depth-first
//                     walk of the implicit tree per wave (the wave's 64 queries are neighbours), entering a box when the squared
//                     distance of any lane's query to it is below that lane's current third best
//    No host read.  Cost per query: the nodes whose box reaches into the query's 3-NN ball and their siblings, independent of how the
//    density varies elsewhere; no quadratic fallback exists.
// 2. lidargs_voxelize_sample: np.unique(np.round(data / voxel_size), axis=0) * voxel_size on the device.
//      k_vx_keys      q = rint(x / v) in the input's precision (correctly rounded division, half to even), as int64; min / max per
//                     axis and a flag for rows the int64 cannot hold (non-finite, |q| >= 2^62)              [host read: min, max, flag]
//      sort           key = (qx - minx, qy - miny, qz - minz) packed MSB-first into as many bits as the spans need, LSD radix over
//                     its 32-bit words (two when it fits 64 bits, up to six)
//      k_vx_heads     a row starts a group if its key differs from the previous row's in sorted order; exclusive scan
//                                                                                                            [host read: count]
//      k_vx_emit      group r -> out[r] = q * v in the input's precision
// Both built with -ffp-contract=off: every squared distance and every quotient rounds as written.
#include "lidargs_common.h"
#include "../../include/lidargs_rasterizer.h"
#include "../../include/lidargs_knn.h"
#include <float.h>
#include <limits.h>
#include <math.h>
#include <string.h>
#include <algorithm>

namespace lg {

#define KNN_FAN 32           // points per leaf, children per inner node (5 bits of a leaf index per level)
#define KNN_LOG_FAN 5
#define KNN_MAX_LEVELS 8     // P <= 2^30: 2^25 leaves, then 2^20, 2^15, 2^10, 2^5 nodes
#define KNN_MAX_P (1 << 30)

struct KnnCenter { double sum[3]; unsigned long long count; };

__device__ __forceinline__ bool knn_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__global__ void __launch_bounds__(256) k_knn_center(int P, const float* __restrict__ pts, int stride, KnnCenter* __restrict__ c) {
    double s[3] = {0.0, 0.0, 0.0};
    unsigned n = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
        const float* p = pts + (size_t)i * stride;
        const float x = p[0], y = p[1], z = p[2];
        if (knn_finite(x, y, z)) { s[0] += x; s[1] += y; s[2] += z; n++; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s[0] += __shfl_xor(s[0], o); s[1] += __shfl_xor(s[1], o); s[2] += __shfl_xor(s[2], o); n += __shfl_xor(n, o);
    }
    if ((threadIdx.x & 63) == 0 && n) {
        atomicAdd(&c->sum[0], s[0]); atomicAdd(&c->sum[1], s[1]); atomicAdd(&c->sum[2], s[2]);
        atomicAdd(&c->count, (unsigned long long)n);
    }
}

// top 21 bits of the order-preserving image of a float (x < y => image(x) <= image(y) after the cut)
__device__ __forceinline__ uint32_t knn_axis_bits(float x) {
    const uint32_t u = __float_as_uint(x);
    return ((u & 0x80000000u) ? ~u : (u | 0x80000000u)) >> 11;
}
__device__ __forceinline__ unsigned long long knn_spread(uint32_t v) {     // 21 bits -> every third bit of 63
    unsigned long long x = v & 0x1FFFFFull;
    x = (x | x << 32) & 0x1F00000000FFFFull;
    x = (x | x << 16) & 0x1F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ void __launch_bounds__(256) k_knn_keys(int P, const float* __restrict__ pts, int stride, const KnnCenter* __restrict__ c,
                                                  uint32_t* __restrict__ key_lo, uint32_t* __restrict__ key_hi, uint32_t* __restrict__ ident) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float* p = pts + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    unsigned long long key = ~0ull;
    if (knn_finite(x, y, z)) {
        const double n = c->count ? (double)c->count : 1.0;
        const float cx = (float)(c->sum[0] / n), cy = (float)(c->sum[1] / n), cz = (float)(c->sum[2] / n);
        key = knn_spread(knn_axis_bits(x - cx)) << 2 | knn_spread(knn_axis_bits(y - cy)) << 1 | knn_spread(knn_axis_bits(z - cz));
    }
    key_lo[i] = (uint32_t)key;
    key_hi[i] = (uint32_t)(key >> 32);
    ident[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) k_knn_gather_hi(int P, const uint32_t* __restrict__ key_hi, const uint32_t* __restrict__ perm, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P) out[i] = key_hi[perm[i]];
}

// Box of every group of KNN_FAN consecutive lanes (a half-wave).  Empty boxes stay (+inf, -inf): their distance to any finite query is +inf.
__device__ __forceinline__ void knn_group_box(float4& lo, float4& hi) {
#pragma unroll
    for (int o = KNN_FAN / 2; o > 0; o >>= 1) {
        lo.x = fminf(lo.x, __shfl_xor(lo.x, o)); lo.y = fminf(lo.y, __shfl_xor(lo.y, o)); lo.z = fminf(lo.z, __shfl_xor(lo.z, o));
        hi.x = fmaxf(hi.x, __shfl_xor(hi.x, o)); hi.y = fmaxf(hi.y, __shfl_xor(hi.y, o)); hi.z = fmaxf(hi.z, __shfl_xor(hi.z, o));
    }
}

__global__ void __launch_bounds__(256) k_knn_leaves(int P, const float* __restrict__ pts, int stride, const uint32_t* __restrict__ perm,
                                                    float4* __restrict__ spts, float4* __restrict__ box) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.0f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
    if (s < P) {
        const float* p = pts + (size_t)perm[s] * stride;
        const float4 q = make_float4(p[0], p[1], p[2], 0.0f);
        spts[s] = q;
        if (knn_finite(q.x, q.y, q.z)) { lo = q; hi = q; lo.w = hi.w = 0.0f; }
    }
    knn_group_box(lo, hi);
    if ((s & (KNN_FAN - 1)) == 0 && s < P) { box[2 * (size_t)(s >> KNN_LOG_FAN)] = lo; box[2 * (size_t)(s >> KNN_LOG_FAN) + 1] = hi; }
}

__global__ void __launch_bounds__(256) k_knn_parents(int n_child, const float4* __restrict__ child, float4* __restrict__ parent) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.0f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
    if (c < n_child) { lo = child[2 * (size_t)c]; hi = child[2 * (size_t)c + 1]; }
    knn_group_box(lo, hi);
    if ((c & (KNN_FAN - 1)) == 0 && c < n_child) { parent[2 * (size_t)(c >> KNN_LOG_FAN)] = lo; parent[2 * (size_t)(c >> KNN_LOG_FAN) + 1] = hi; }
}

// Squared distance from q to the box, a lower bound of the squared distance to every point inside, EXACT in float32: for p.x >= lo.x > q.x,
// fl(lo.x - q.x) <= fl(p.x - q.x) (rounding is monotone), likewise fl(q.x - hi.x) <= fl(q.x - p.x) = -fl(p.x - q.x), and squaring
// non-negative values and adding them in the same order keep the inequality.  Without contraction (this file is built with
// -ffp-contract=off) the point's distance below is evaluated with exactly those roundings, so a box is skipped only if none of its
// points can have a squared distance below the current third best.
__device__ __forceinline__ float knn_box_dist(const float4& q, const float4& lo, const float4& hi) {
    const float dx = q.x < lo.x ? lo.x - q.x : (q.x > hi.x ? q.x - hi.x : 0.0f);
    const float dy = q.y < lo.y ? lo.y - q.y : (q.y > hi.y ? q.y - hi.y : 0.0f);
    const float dz = q.z < lo.z ? lo.z - q.z : (q.z > hi.z ? q.z - hi.z : 0.0f);
    return dx * dx + dy * dy + dz * dz;
}
// Candidate j of query q: d = dx*dx + dy*dy + dz*dz with dx = p_j.x - q.x, as the contract writes it.  Only d < b2 enters, so d >= FLT_MAX,
// +inf and NaN (a non-finite point) never do, and a tie with the third best leaves the multiset unchanged.
__device__ __forceinline__ void knn_offer(const float4& q, const float4& pj, float& b0, float& b1, float& b2) {
    const float dx = pj.x - q.x, dy = pj.y - q.y, dz = pj.z - q.z;
    const float d = dx * dx + dy * dy + dz * dz;
    if (d < b2) {                                                      // insert into the sorted three (min / max: no branches, no indexed array)
        const float x0 = fmaxf(b0, d), x1 = fmaxf(b1, x0);
        b0 = fminf(b0, d); b1 = fminf(b1, x0); b2 = fminf(b2, x1);
    }
}
__device__ __forceinline__ int knn_level_nodes(int P, int level) { return ((P - 1) >> (KNN_LOG_FAN * (level + 1))) + 1; }

struct KnnTree { int P, top; int off[KNN_MAX_LEVELS]; };       // off: first box of each level in the box array (leaves first)

// One walk per WAVE: the 64 queries are neighbours in key order, so the nodes they need overlap.  A node is entered when any lane's bound
// reaches it (a ballot), so the walk's position is wave-uniform: box and point loads are broadcasts and no lane waits on another's leaf
// scan (a walk per lane measured 82 ms for 4 M points: the desynchronised lanes made every step of the wave cost a full leaf scan).  Each
// lane still offers only the points of leaves its own bound reaches -- entering a node for another lane costs time, never a result.
__global__ void __launch_bounds__(256) k_knn_query(KnnTree t, const float4* __restrict__ spts, const float4* __restrict__ box,
                                                   const uint32_t* __restrict__ perm, float* __restrict__ out) {
    __shared__ int s_off[KNN_MAX_LEVELS];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l < KNN_MAX_LEVELS; l++) s_off[l] = t.off[l];
    }
    __syncthreads();
    const int s = blockIdx.x * 256 + threadIdx.x;
    const float4 q = s < t.P ? spts[s] : make_float4(NAN, NAN, NAN, 0.0f);
    const bool active = knn_finite(q.x, q.y, q.z);                     // (s >= P reads as NaN: inactive)
    float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;
    const int own = s >> KNN_LOG_FAN;
    if (active) {
        // seed: every other point of the query's own leaf (neighbours in key order: the bound is tight before the walk starts)
        const int j0 = own << KNN_LOG_FAN, j1 = min(j0 + KNN_FAN, t.P);
        for (int j = j0; j < j1; j++)
            if (j != s) knn_offer(q, spts[j], b0, b1, b2);
    }
    if (__any(active)) {
        // stackless depth-first walk: a node is (level, index), its children are index * KNN_FAN + [0, KNN_FAN) one level down
        int level = t.top, idx = 0;
        const int n_top = knn_level_nodes(t.P, t.top);
        for (;;) {
            const size_t b = 2 * (size_t)(s_off[level] + idx);
            const bool want = active && !(level == 0 && idx == own) && knn_box_dist(q, box[b], box[b + 1]) < b2;
            const bool in = __any(want);
            if (in && level > 0) { level--; idx <<= KNN_LOG_FAN; continue; }
            if (in && want) {
                const int e = min((idx + 1) << KNN_LOG_FAN, t.P);
                for (int j = idx << KNN_LOG_FAN; j < e; j++) knn_offer(q, spts[j], b0, b1, b2);
            }
            // next node: the next sibling, or the parent's next sibling once the siblings are done
            for (;;) {
                idx++;
                if (level == t.top) break;
                if ((idx & (KNN_FAN - 1)) != 0 && idx < knn_level_nodes(t.P, level)) break;
                idx = (idx - 1) >> KNN_LOG_FAN;
                level++;
            }
            if (level == t.top && idx >= n_top) break;
        }
    }
    if (s < t.P) out[perm[s]] = ((b0 + b1) + b2) / 3.0f;               // correctly rounded (hipcc's default for float division)
}

// ---- voxelize_sample ------------------------------------------------------------------------------------------------------------
#define VX_HDR_WORDS 16      // u32 words: [0..5] int64 min xyz, [6..11] int64 max xyz, [12] bad rows
#define VX_Q_LIMIT 4611686018427387904.0      // 2^62: |q| below it keeps every span inside 63 bits

template <typename T> __device__ __forceinline__ T vx_rint(T x);
template <> __device__ __forceinline__ float vx_rint<float>(float x) { return __builtin_rintf(x); }
template <> __device__ __forceinline__ double vx_rint<double>(double x) { return __builtin_rint(x); }

__global__ void k_vx_init(long long* hdr) {
    const int t = threadIdx.x;
    if (t < 3) { hdr[t] = LLONG_MAX; hdr[3 + t] = LLONG_MIN; }
    if (t == 0) hdr[6] = 0;
}

template <typename T>
__global__ void __launch_bounds__(256) k_vx_keys(int P, const T* __restrict__ pts, T v, long long* __restrict__ q, long long* __restrict__ hdr) {
    long long lo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, hi[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN};
    long long bad = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const T r = vx_rint<T>(pts[3 * (size_t)i + c] / v);        // np.round(data / voxel_size): IEEE quotient, half to even
            long long k = 0;
            if (fabs((double)r) < VX_Q_LIMIT) k = (long long)r;        // an integer-valued float: exact
            else bad = 1;                                              // NaN, inf, or beyond the key range
            q[3 * (size_t)i + c] = k;
            lo[c] = min(lo[c], k); hi[c] = max(hi[c], k);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[c] = min(lo[c], (long long)__shfl_xor(lo[c], o)); hi[c] = max(hi[c], (long long)__shfl_xor(hi[c], o)); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad |= (long long)__shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) { atomicMin(&hdr[c], lo[c]); atomicMax(&hdr[3 + c], hi[c]); }
        if (bad) atomicOr((unsigned long long*)&hdr[6], 1ull);
    }
}

struct VxKey { long long mn[3]; int bits[3]; int shift[3]; };     // key = (qx - mnx) << shift[0] | (qy - mny) << shift[1] | (qz - mnz)

// bits [32 w, 32 w + 32) of the packed key
__device__ __forceinline__ uint32_t vx_word(const VxKey& kd, const long long* qr, int w) {
    uint32_t r = 0;
    const int lo = 32 * w;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (kd.bits[c] == 0) continue;
        const unsigned long long u = (unsigned long long)(qr[c] - kd.mn[c]);      // < 2^63
        const int a = kd.shift[c], e = a + kd.bits[c];                            // the axis' bits [a, e) of the key
        if (e <= lo || a >= lo + 32) continue;
        if (a >= lo) r |= (uint32_t)(u << (a - lo));                               // a - lo < 32
        else r |= (uint32_t)(u >> (lo - a));                                       // lo - a < 64 (bits <= 63)
    }
    return r;
}

__global__ void __launch_bounds__(256) k_vx_word(int P, VxKey kd, const long long* __restrict__ q, const uint32_t* __restrict__ perm, int w,
                                                 uint32_t* __restrict__ out, uint32_t* __restrict__ ident) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const uint32_t r = perm ? perm[i] : (uint32_t)i;
    out[i] = vx_word(kd, q + 3 * (size_t)r, w);
    if (ident) ident[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) k_vx_heads(int P, const long long* __restrict__ q, const uint32_t* __restrict__ perm, uint32_t* __restrict__ head) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    uint32_t h = 1;
    if (i > 0) {
        const long long* a = q + 3 * (size_t)perm[i];
        const long long* b = q + 3 * (size_t)perm[i - 1];
        h = (a[0] != b[0] || a[1] != b[1] || a[2] != b[2]) ? 1u : 0u;
    }
    head[i] = h;
}

template <typename T>
__global__ void __launch_bounds__(256) k_vx_emit(int P, const long long* __restrict__ q, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ head,
                                                 const uint32_t* __restrict__ pos, T v, T* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P || !head[i]) return;
    const long long* a = q + 3 * (size_t)perm[i];
    const size_t r = pos[i];
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * r + c] = (T)a[c] * v;             // the rounded quotient is an integer of the input's type: exact
}

}  // namespace lg

#define KNN_HIP(call) do { hipError_t e_ = (hipError_t)(call); if (e_ != hipSuccess) return lg::api_fail(LIDARGS_ERR_HIP, hipGetErrorString(e_)); } while (0)

namespace {
int knn_levels(int P, int off[KNN_MAX_LEVELS], size_t* total_nodes) {
    int top = 0, acc = 0;
    for (int l = 0; l < KNN_MAX_LEVELS; l++) off[l] = 0;
    for (int l = 0;; l++) {
        const int n = ((P - 1) >> (KNN_LOG_FAN * (l + 1))) + 1;
        off[l] = acc; acc += n; top = l;
        if (n <= KNN_FAN) break;
    }
    *total_nodes = (size_t)acc;
    return top;
}
struct KnnCarve { lg::KnnCenter* center; uint32_t *ka, *kb, *va, *vb, *hi, *sort; float4* spts; float4* box; };
size_t knn_carve(int P, char* base, KnnCarve* c) {
    int off[KNN_MAX_LEVELS]; size_t nodes = 0;
    knn_levels(P, off, &nodes);
    lg::Carver cv(base);
    c->center = cv.take<lg::KnnCenter>(1);
    c->ka = cv.take<uint32_t>(P); c->kb = cv.take<uint32_t>(P); c->va = cv.take<uint32_t>(P); c->vb = cv.take<uint32_t>(P);
    c->hi = cv.take<uint32_t>(P);
    c->sort = cv.take<uint32_t>(lg::sort_scratch_words(P, lg::SORT_MAX_RADIX_BITS));
    c->spts = cv.take<float4>(P);
    c->box = cv.take<float4>(2 * nodes);
    return (size_t)(cv.p - base) + 128;
}
}  // namespace

extern "C" {

size_t lidargs_knn_scratch_bytes(int P) {
    if (P < 1 || P > KNN_MAX_P) return 0;
    KnnCarve c;
    return knn_carve(P, nullptr, &c);
}

int lidargs_knn_mean_dist(int P, const float* points, int row_stride, float* out, char* scratch, size_t scratch_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || P > KNN_MAX_P) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "knn_mean_dist: P must be in [0, 2^30]");
    if (row_stride < 3) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "knn_mean_dist: row_stride must be at least 3 floats");
    if ((size_t)P * row_stride >= ((size_t)1 << 40)) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "knn_mean_dist: P * row_stride too large");
    if (P == 0) return 0;
    if (!points || !out || !scratch) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "knn_mean_dist: NULL pointer");
    if (scratch_bytes < lidargs_knn_scratch_bytes(P)) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "knn_mean_dist: scratch too small");
    KnnCarve c;
    knn_carve(P, scratch, &c);
    lg::KnnTree t;
    size_t nodes = 0;
    t.P = P; t.top = knn_levels(P, t.off, &nodes);
    const unsigned pb = (unsigned)((P + 255) / 256);

    KNN_HIP(hipMemsetAsync(c.center, 0, sizeof(lg::KnnCenter), stream));
    hipLaunchKernelGGL(lg::k_knn_center, dim3(std::min(pb, 1024u)), dim3(256), 0, stream, P, points, row_stride, c.center);
    hipLaunchKernelGGL(lg::k_knn_keys, dim3(pb), dim3(256), 0, stream, P, points, row_stride, c.center, c.ka, c.hi, c.va);
    // 64-bit key order: LSD on the low word (values = rows), then on the high word gathered through that permutation
    int side = lg::launch_radix_sort_pairs(c.ka, c.kb, c.va, c.vb, P, 32, c.sort, stream, lg::SORT_MAX_RADIX_BITS, nullptr, 0, true);
    uint32_t* perm = side ? c.vb : c.va;
    uint32_t* other = side ? c.va : c.vb;
    hipLaunchKernelGGL(lg::k_knn_gather_hi, dim3(pb), dim3(256), 0, stream, P, c.hi, perm, c.ka);
    side = lg::launch_radix_sort_pairs(c.ka, c.kb, perm, other, P, 32, c.sort, stream, lg::SORT_MAX_RADIX_BITS);
    perm = side ? other : perm;
    KNN_HIP(hipGetLastError());

    hipLaunchKernelGGL(lg::k_knn_leaves, dim3(pb), dim3(256), 0, stream, P, points, row_stride, perm, c.spts, c.box);
    for (int l = 1; l <= t.top; l++) {
        const int n_child = ((P - 1) >> (KNN_LOG_FAN * l)) + 1;
        hipLaunchKernelGGL(lg::k_knn_parents, dim3((unsigned)((n_child + 255) / 256)), dim3(256), 0, stream, n_child,
                           c.box + 2 * (size_t)t.off[l - 1], c.box + 2 * (size_t)t.off[l]);
    }
    hipLaunchKernelGGL(lg::k_knn_query, dim3(pb), dim3(256), 0, stream, t, c.spts, c.box, perm, out);
    KNN_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

namespace {
struct VxCarve { long long* hdr; long long* q; uint32_t *ka, *kb, *va, *vb, *head, *pos, *total, *sort, *scan; };
size_t vx_carve(int P, char* base, VxCarve* c) {
    lg::Carver cv(base);
    c->hdr = cv.take<long long>(VX_HDR_WORDS / 2);
    c->q = cv.take<long long>(3 * (size_t)P);
    c->ka = cv.take<uint32_t>(P); c->kb = cv.take<uint32_t>(P); c->va = cv.take<uint32_t>(P); c->vb = cv.take<uint32_t>(P);
    c->head = cv.take<uint32_t>(P); c->pos = cv.take<uint32_t>(P); c->total = cv.take<uint32_t>(1);
    c->sort = cv.take<uint32_t>(lg::sort_scratch_words(P, lg::SORT_MAX_RADIX_BITS));
    c->scan = cv.take<uint32_t>(lg::scan_scratch_words(P));
    return (size_t)(cv.p - base) + 128;
}
template <typename T>
int vx_run(int P, const T* points, T v, const VxCarve& c, lidargs_alloc_fn alloc_out, void* out_user, hipStream_t stream) {
    const unsigned pb = (unsigned)((P + 255) / 256);
    hipLaunchKernelGGL(lg::k_vx_init, dim3(1), dim3(64), 0, stream, c.hdr);
    hipLaunchKernelGGL(lg::k_vx_keys<T>, dim3(std::min(pb, 1024u)), dim3(256), 0, stream, P, points, v, c.q, c.hdr);
    KNN_HIP(hipGetLastError());
    uint32_t h[14];
    KNN_HIP(lg::api_read_words_zero_behind((const uint32_t*)c.hdr, 14, h, nullptr, 0, stream));
    long long hv[7];
    memcpy(hv, h, sizeof(hv));
    if (hv[6]) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "voxelize_sample: a row is not finite, or data / voxel_size reaches 2^62");
    lg::VxKey kd;
    int total = 0;
    for (int a = 2; a >= 0; a--) {                                     // z least significant: the key's order is the rows' lexicographic order
        kd.mn[a] = hv[a];
        const unsigned long long span = (unsigned long long)(hv[3 + a] - hv[a]);
        int b = 0;
        while (b < 63 && (span >> b) != 0) b++;
        kd.bits[a] = b; kd.shift[a] = total; total += b;
    }
    const int words = (total + 31) / 32;
    uint32_t* vbuf[2] = {c.va, c.vb};
    int cur = 0;
    for (int w = 0; w < words; w++) {
        const int end_bit = std::min(32, total - 32 * w);
        hipLaunchKernelGGL(lg::k_vx_word, dim3(pb), dim3(256), 0, stream, P, kd, c.q, w ? vbuf[cur] : (const uint32_t*)nullptr, w, c.ka,
                           w ? (uint32_t*)nullptr : vbuf[cur]);
        const int side = lg::launch_radix_sort_pairs(c.ka, c.kb, vbuf[cur], vbuf[1 - cur], P, end_bit, c.sort, stream, lg::SORT_MAX_RADIX_BITS,
                                                     nullptr, 0, w == 0);
        if (side) cur = 1 - cur;
    }
    const uint32_t* perm = words ? vbuf[cur] : nullptr;
    if (!perm) {                                                       // every row in the same voxel: the identity order
        hipLaunchKernelGGL(lg::k_vx_word, dim3(pb), dim3(256), 0, stream, P, kd, c.q, (const uint32_t*)nullptr, 0, c.ka, c.va);
        perm = c.va;
    }
    hipLaunchKernelGGL(lg::k_vx_heads, dim3(pb), dim3(256), 0, stream, P, c.q, perm, c.head);
    lg::launch_exclusive_scan(c.head, c.pos, P, c.total, c.scan, stream);
    KNN_HIP(hipGetLastError());
    uint32_t U = 0;
    KNN_HIP(lg::api_read_words_zero_behind(c.total, 1, &U, nullptr, 0, stream));
    T* out = (T*)alloc_out(out_user, (size_t)U * 3 * sizeof(T));
    if (!out) return lg::api_fail(LIDARGS_ERR_ALLOC, "voxelize_sample: the output allocator returned NULL");
    hipLaunchKernelGGL(lg::k_vx_emit<T>, dim3(pb), dim3(256), 0, stream, P, c.q, perm, c.head, c.pos, v, out);
    KNN_HIP(hipGetLastError());
    return (int)U;
}
}  // namespace

extern "C" {

size_t lidargs_voxelize_scratch_bytes(int P) {
    if (P < 1 || P > KNN_MAX_P) return 0;
    VxCarve c;
    return vx_carve(P, nullptr, &c);
}

int lidargs_voxelize_sample(int P, const void* points, int is_double, double voxel_size, char* scratch, size_t scratch_bytes,
                            lidargs_alloc_fn alloc_out, void* out_user, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || P > KNN_MAX_P) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "voxelize_sample: P must be in [0, 2^30]");
    const bool ok_v = is_double ? (voxel_size > 0.0 && voxel_size < (double)INFINITY) : ((float)voxel_size > 0.0f && (float)voxel_size < INFINITY);
    if (!ok_v) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "voxelize_sample: voxel_size must be positive and finite in the data's precision");
    if (!alloc_out) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "voxelize_sample: NULL allocator");
    if (P == 0) return 0;                                              // no rows: nothing is allocated
    if (!points || !scratch) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "voxelize_sample: NULL pointer");
    if (scratch_bytes < lidargs_voxelize_scratch_bytes(P)) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "voxelize_sample: scratch too small");
    VxCarve c;
    vx_carve(P, scratch, &c);
    if (is_double) return vx_run<double>(P, (const double*)points, voxel_size, c, alloc_out, out_user, stream);
    return vx_run<float>(P, (const float*)points, (float)voxel_size, c, alloc_out, out_user, stream);
}

}  // extern "C"
