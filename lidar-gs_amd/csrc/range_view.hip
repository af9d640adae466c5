// range_view.hip -- point cloud <-> range image on the device (include_rangeview/lidargs_range_view.h; DESIGN.md section "Range view").
// The only source of liblidargs_rangeview.so: nothing here is linked into liblidargs_hip.so, and nothing of chamfer.hip is used -- the
// few lines of ray math the points meter has (k_pm_points) are restated in pixel_dir below.
//
// project (utils/lidar_utils.py:51-110), three launches:
//   k_rv_fill      every 64-bit pixel key = all ones
//   k_rv_project   one lane per point, grid-stride: range, column, row in float32 as the reference evaluates them, then
//                  atomicMin(key[pixel], (bits(dist) << 32) | index).  dist > 0 and finite, so its bits order like the float; the index in
//                  the low word makes the first point in input order win among equal ranges -- what the reference's sequential loop
//                  (`pano == 0 or pano > dist`) leaves in the pixel.  All ones is no key of a point (its high word is a NaN).
//   k_rv_resolve   one lane per pixel: empty -> (0, 0), else (dist of the key, intensity of the key's point)
// unproject (:171-214), three launches, no flag array: the flag `pano != 0` is one compare, so it is taken twice instead of stored
//   k_rv_count     one workgroup per tile of RV_TILE consecutive pixels -> the tile's number of non-empty pixels
//   k_rv_scan      ONE workgroup: exclusive prefix of the tile counts in place, the total to out_count
//   k_rv_points    per tile again: prefix inside the tile (wave shuffles + one LDS round), each non-empty pixel writes its row
// Built with -ffp-contract=off: the row and column decisions are compared pixel for pixel with the reference's float32 evaluation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include_rangeview/lidargs_range_view.h"
#include "lidargs_status.h"

namespace {

constexpr int RV_THREADS = 256;
constexpr int RV_PER_THREAD = 4;                           // consecutive pixels of one thread: thread order is pixel order
constexpr int RV_TILE = RV_THREADS * RV_PER_THREAD;
constexpr long long RV_MAX_PIXELS = 1ll << 28;
constexpr int RV_PROJECT_MAX_BLOCKS = 2048;                // k_rv_project: 256 CUs x 8 workgroups (8 waves a SIMD); beyond 524 288 points, grid-stride rounds
constexpr float PI_F = 3.14159265358979323846f;            // np.float32(np.pi)
constexpr unsigned long long RV_EMPTY = ~0ull;

struct Xform { double m[12]; int on; };                    // 3x4 row-major [R | t]; travels in the kernel argument

// the row rule in float32; fov mode: c_down = (float)((fov - fov_up) / 180 * pi), row_step = (float)(fov / 180 * pi / H)
struct Rows { const float* beams; float fov_up, fov, c_down, row_step; };

__device__ __forceinline__ float3 apply(const Xform& t, float x, float y, float z) {
    if (!t.on) return make_float3(x, y, z);
    const double X = x, Y = y, Z = z;
    return make_float3((float)(((t.m[0] * X + t.m[1] * Y) + t.m[2] * Z) + t.m[3]), (float)(((t.m[4] * X + t.m[5] * Y) + t.m[6] * Z) + t.m[7]),
                       (float)(((t.m[8] * X + t.m[9] * Y) + t.m[10] * Z) + t.m[11]));
}

__global__ void __launch_bounds__(RV_THREADS) k_rv_fill(int n, unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * RV_THREADS + threadIdx.x;
    if (i < n) keys[i] = RV_EMPTY;
}

// find_closest_label (:33-49): the NEAREST beam; on a tie `after - a < a - before` is false, the lower beam; clamped at both ends
__device__ __forceinline__ int nearest_beam(const float* __restrict__ beams, int H, float a) {
    if (H == 1 || a >= beams[H - 1]) return H - 1;
    if (a <= beams[0]) return 0;
    int lo = 0, hi = H;                                    // bisect_left: the first pos with beams[pos] >= a; here 1 <= pos <= H - 1
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (beams[mid] < a) lo = mid + 1; else hi = mid;
    }
    lo = lo < 1 ? 1 : (lo > H - 1 ? H - 1 : lo);          // (no change for an ascending table; a table that is not must not read outside)
    const float before = beams[lo - 1], after = beams[lo];
    return (after - a < a - before) ? lo : lo - 1;
}

__global__ void __launch_bounds__(RV_THREADS) k_rv_project(int N, const float4* __restrict__ points, int H, int W, Rows rows, float col_step,
                                                           float max_depth, Xform xf, int flags, unsigned long long* keys) {
    const long long stride = (long long)gridDim.x * RV_THREADS;
    for (long long i = (long long)blockIdx.x * RV_THREADS + threadIdx.x; i < N; i += stride) {
        const float4 p = points[i];
        const float3 q = apply(xf, p.x, p.y, p.z);
        const float x = q.x, y = q.y, z = q.z;
        const float dist = sqrtf((x * x + y * y) + z * z);                 // np.linalg.norm of a float32 row
        if (!(isfinite(x) && isfinite(y) && isfinite(z) && isfinite(p.w) && isfinite(dist))) continue;
        if (dist >= max_depth || dist == 0.0f) continue;
        const float beta = PI_F - atan2f(y, x);
        const float cf = rintf(beta / col_step);                           // Python's round(): ties to even
        if (!(cf >= 0.0f && cf <= (float)W)) continue;
        int c = (int)cf;
        if (c == W) {                                                      // azimuth -pi: the same ray as +pi
            if (!(flags & LIDARGS_RV_PIXEL_ROWS)) continue;
            c = 0;
        }
        const float a = atan2f(z, sqrtf(x * x + y * y));
        int r;
        if (rows.beams) {
            const int label = nearest_beam(rows.beams, H, a);
            r = (flags & LIDARGS_RV_PIXEL_ROWS) ? H - 1 - label : H - label;
        } else {
            const float rf = rintf((float)H - (a + rows.c_down) / rows.row_step);
            if (!(rf >= 0.0f && rf < (float)H)) continue;
            r = (int)rf;
        }
        if (r < 0 || r >= H) continue;
        unsigned long long* slot = keys + (size_t)r * W + c;
        const unsigned long long key = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)i;
        // a key only ever decreases, so a point that does not beat what a relaxed load sees (the current key or an older, larger one)
        // cannot win: with many contenders per pixel most points stop here and the atomic units see only the running minima
        if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(slot, key);
    }
}

__global__ void __launch_bounds__(RV_THREADS) k_rv_resolve(int n, const unsigned long long* __restrict__ keys, const float* __restrict__ points,
                                                           float* __restrict__ pano, float* __restrict__ intensity) {
    const int i = blockIdx.x * RV_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    const bool hit = k != RV_EMPTY;
    pano[i] = hit ? __uint_as_float((unsigned)(k >> 32)) : 0.0f;
    intensity[i] = hit ? points[4 * (size_t)(unsigned)k + 3] : 0.0f;
}

// utils/lidar_utils.py:186-199 in float32, operation by operation; cos / sin correctly rounded (through double)
__device__ __forceinline__ float3 pixel_dir(int row, int col, int H, int W, const Rows& rows) {
    const float beta = ((-((float)col - (float)W / 2.0f)) / (float)W) * 2.0f * PI_F;
    float alpha;
    if (rows.beams) alpha = rows.beams[H - 1 - row];                       // beam_inclinations[::-1][j]
    else alpha = ((rows.fov_up - (float)row / (float)H * rows.fov) / 180.0f) * PI_F;
    const float ca = (float)cos((double)alpha), sa = (float)sin((double)alpha), cb = (float)cos((double)beta), sb = (float)sin((double)beta);
    return make_float3(ca * cb, ca * sb, sa);
}

__global__ void __launch_bounds__(RV_THREADS) k_rv_ray_dirs(int H, int W, Rows rows, float* __restrict__ out) {
    const int i = blockIdx.x * RV_THREADS + threadIdx.x;
    if (i >= H * W) return;
    const int row = i / W, col = i - row * W;
    const float3 d = pixel_dir(row, col, H, W, rows);
    out[3 * (size_t)i] = d.x; out[3 * (size_t)i + 1] = d.y; out[3 * (size_t)i + 2] = d.z;
}

// inclusive prefix of v over the workgroup's 256 threads (four waves of 64); `total` is the workgroup's sum.  s: 4 words of LDS.
__device__ __forceinline__ unsigned block_inclusive_scan(unsigned v, unsigned* s, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    __syncthreads();                                       // (s may still be read from the previous call)
    if (lane == 63) s[wave] = v;
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < 4; w++) before += w < wave ? s[w] : 0u;
    total = s[0] + s[1] + s[2] + s[3];
    return v + before;
}

__global__ void __launch_bounds__(RV_THREADS) k_rv_count(int n, const float* __restrict__ pano, unsigned* __restrict__ tile_count) {
    __shared__ unsigned s[4];
    const long long base = (long long)blockIdx.x * RV_TILE + threadIdx.x * RV_PER_THREAD;
    unsigned v = 0;
    for (int k = 0; k < RV_PER_THREAD; k++) if (base + k < n) v += pano[base + k] != 0.0f ? 1u : 0u;
    unsigned total;
    block_inclusive_scan(v, s, total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

__global__ void __launch_bounds__(RV_THREADS) k_rv_scan(int tiles, unsigned* __restrict__ tile_count, unsigned* __restrict__ out_count) {
    __shared__ unsigned s[4];
    unsigned carry = 0;
    for (int b = 0; b < tiles; b += RV_THREADS) {          // (uniform trip count: every thread reaches the barriers)
        const int i = b + threadIdx.x;
        const unsigned v = i < tiles ? tile_count[i] : 0u;
        unsigned total;
        const unsigned incl = block_inclusive_scan(v, s, total);
        if (i < tiles) tile_count[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) *out_count = carry;
}

__global__ void __launch_bounds__(RV_THREADS) k_rv_points(int H, int W, const float* __restrict__ pano, const float* __restrict__ intensity, Rows rows,
                                                          Xform xf, const unsigned* __restrict__ tile_offset, float4* __restrict__ out) {
    __shared__ unsigned s[4];
    const int n = H * W;
    const long long base = (long long)blockIdx.x * RV_TILE + threadIdx.x * RV_PER_THREAD;
    float d[RV_PER_THREAD];
    unsigned v = 0;
    for (int k = 0; k < RV_PER_THREAD; k++) {
        d[k] = base + k < n ? pano[base + k] : 0.0f;
        v += d[k] != 0.0f ? 1u : 0u;
    }
    unsigned total;
    unsigned at = tile_offset[blockIdx.x] + block_inclusive_scan(v, s, total) - v;
    for (int k = 0; k < RV_PER_THREAD; k++) {
        if (!(d[k] != 0.0f)) continue;
        const int pix = (int)(base + k), row = pix / W, col = pix - row * W;
        const float3 u = pixel_dir(row, col, H, W, rows);
        const float3 q = apply(xf, u.x * d[k], u.y * d[k], u.z * d[k]);
        out[at++] = make_float4(q.x, q.y, q.z, intensity ? intensity[pix] : 0.0f);
    }
}

// 0, or the message of what is wrong with the image size and the row rule
const char* check_rows(int H, int W, const float* beams, float fov) {
    if (H <= 0 || W <= 0 || (long long)H * W > RV_MAX_PIXELS) return "bad image size";
    if (!beams && !(fov > 0.0f && isfinite(fov))) return "without a beam table fov must be positive";
    return nullptr;
}

Rows make_rows(int H, const float* beams, float fov_up, float fov) {
    const double pi = 3.141592653589793;
    // the reference's Python doubles: fov_down / 180 * np.pi and fov / 180 * np.pi / lidar_H, each rounded to float32 where it meets one
    return Rows{beams, fov_up, fov, (float)(((double)fov - (double)fov_up) / 180 * pi), (float)((double)fov / 180 * pi / H)};
}

Xform make_xform(const double* m) {
    Xform t;
    t.on = m != nullptr;
    for (int i = 0; i < 12; i++) t.m[i] = m ? m[i] : 0.0;
    return t;
}

int blocks_for(long long n) { return (int)((n + RV_THREADS - 1) / RV_THREADS); }

}  // namespace

extern "C" {

int lidargs_rv_abi_version(void) { return LIDARGS_RV_ABI_VERSION; }
const char* lidargs_rv_last_error(void) { return g_err; }

size_t lidargs_rv_scratch_bytes(int H, int W) {
    if (H <= 0 || W <= 0 || (long long)H * W > RV_MAX_PIXELS) return 0;
    return (size_t)H * W * sizeof(unsigned long long) + 256;               // the pixel keys; the tile counts of unproject are fewer
}

int lidargs_rv_project(int N, const float* points, int H, int W, const float* beams, float fov_up, float fov, float max_depth,
                       const double* world_to_sensor, int flags, float* out_pano, float* out_intensity,
                       char* scratch, size_t scratch_bytes, void* stream_) {
    const char* what = "rv_project";
    hipStream_t stream = (hipStream_t)stream_;
    if (const char* m = check_rows(H, W, beams, fov)) return fail(-1, what, m);
    if (N < 0) return fail(-1, what, "negative N");
    if (flags & ~LIDARGS_RV_PIXEL_ROWS) return fail(-1, what, "unknown flags");
    if ((N > 0 && !points) || !out_pano || !out_intensity || !scratch) return fail(-1, what, "NULL pointer");
    if ((uintptr_t)points & 15) return fail(-1, what, "points must be 16-byte aligned");
    if (scratch_bytes < lidargs_rv_scratch_bytes(H, W) || ((uintptr_t)scratch & 7)) return fail(-1, what, "scratch too small or not 8-byte aligned");
    const int n = H * W;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(scratch);
    hipLaunchKernelGGL(k_rv_fill, dim3(blocks_for(n)), dim3(RV_THREADS), 0, stream, n, keys);
    if (N > 0) {
        const int grid = blocks_for(N) < RV_PROJECT_MAX_BLOCKS ? blocks_for(N) : RV_PROJECT_MAX_BLOCKS;
        hipLaunchKernelGGL(k_rv_project, dim3(grid), dim3(RV_THREADS), 0, stream, N, reinterpret_cast<const float4*>(points), H, W,
                           make_rows(H, beams, fov_up, fov), (float)(2 * 3.141592653589793 / W), max_depth, make_xform(world_to_sensor), flags, keys);
    }
    hipLaunchKernelGGL(k_rv_resolve, dim3(blocks_for(n)), dim3(RV_THREADS), 0, stream, n, keys, points, out_pano, out_intensity);
    return launched(-4, what);
}

int lidargs_rv_unproject(int H, int W, const float* pano, const float* intensity, const float* beams, float fov_up, float fov,
                         const double* sensor_to_world, float* out_points, unsigned* out_count, char* scratch, size_t scratch_bytes, void* stream_) {
    const char* what = "rv_unproject";
    hipStream_t stream = (hipStream_t)stream_;
    if (const char* m = check_rows(H, W, beams, fov)) return fail(-1, what, m);
    if (!pano || !out_points || !out_count || !scratch) return fail(-1, what, "NULL pointer");
    if ((uintptr_t)out_points & 15) return fail(-1, what, "out_points must be 16-byte aligned");
    if (scratch_bytes < lidargs_rv_scratch_bytes(H, W) || ((uintptr_t)scratch & 7)) return fail(-1, what, "scratch too small or not 8-byte aligned");
    const int n = H * W, tiles = (n + RV_TILE - 1) / RV_TILE;
    unsigned* tile_count = reinterpret_cast<unsigned*>(scratch);
    hipLaunchKernelGGL(k_rv_count, dim3(tiles), dim3(RV_THREADS), 0, stream, n, pano, tile_count);
    hipLaunchKernelGGL(k_rv_scan, dim3(1), dim3(RV_THREADS), 0, stream, tiles, tile_count, out_count);
    hipLaunchKernelGGL(k_rv_points, dim3(tiles), dim3(RV_THREADS), 0, stream, H, W, pano, intensity, make_rows(H, beams, fov_up, fov),
                       make_xform(sensor_to_world), tile_count, reinterpret_cast<float4*>(out_points));
    return launched(-4, what);
}

int lidargs_rv_ray_dirs(int H, int W, const float* beams, float fov_up, float fov, float* out_dirs, void* stream_) {
    const char* what = "rv_ray_dirs";
    if (const char* m = check_rows(H, W, beams, fov)) return fail(-1, what, m);
    if (!out_dirs) return fail(-1, what, "NULL pointer");
    hipLaunchKernelGGL(k_rv_ray_dirs, dim3(blocks_for((long long)H * W)), dim3(RV_THREADS), 0, (hipStream_t)stream_, H, W, make_rows(H, beams, fov_up, fov), out_dirs);
    return launched(-4, what);
}

}  // extern "C"
