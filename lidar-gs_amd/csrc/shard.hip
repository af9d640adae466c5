// shard.hip -- the sharded (multi-GPU) path's own kernels and their entry points (gfx950): everything lidargs_dist.py calls around a
// rank's frame.  The frames themselves (lidargs_forward_shell* / _wedge*, lidargs_backward_shell / _wedge, lidargs_render_shell) are
// forward_impl / backward_impl callers and live in api.hip.
//
//   selection    a rank's Gaussians -- range shell [lo, hi) or column wedge [col_lo, col_hi), the tests of selection.h -- gathered
//                into dense rows in ascending index order: flags + scan + gather (k_shell_flags / k_wedge_flags, k_shell_gather), or
//                one launch (k_select_fused)
//   gradients    the rows of the gradient all-to-all: k_shell_pack_rows, k_shell_pack_rows_live, k_shell_unpack_rows(_add),
//                k_shell_chunk_counts (its split sizes), k_shell_scatter_i32 (the radii)
//   images       per-pixel folds over the G shells (k_shell_transmittance, k_shell_compose) and a wedge's pixel columns to and from
//                the block the image all-gather ships (k_wedge_pack_columns, k_wedge_unpack_columns)
//
// Every extern "C" entry point stands next to the kernel it launches, inside namespace lg (C linkage: the function
// include/lidargs_rasterizer.h declares, whatever the namespace).  Rounding: the file is built with the default flags and says per
// part, by pragma, whether a * b + c may fuse -- the selection and the gradient rows round as written (they were compiled so before
// they had a file of their own, and the selection must agree with k_preprocess bit for bit: selection.h), the image folds fuse.
#include "lidargs_common.h"
#include "selection.h"
#include "../../include/lidargs_rasterizer.h"

#include <stdio.h>

namespace lg {

static int hip_fail(const char* call, hipError_t e) {
    char msg[512];
    snprintf(msg, sizeof msg, "%s: %s", call, hipGetErrorString(e));
    return api_fail(LIDARGS_ERR_HIP, msg);
}
#define SH_HIP(call)                                      \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return hip_fail(#call, e_); \
    } while (0)

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// Selection in two steps (so that the caller can allocate exactly M output rows per frame: the selection a forward saves for its
// backward must not be overwritten by the next forward's): flag the Gaussians of the rank's cut, scan the flags, read the total
// (count); then gather their attributes into dense arrays in ascending index order (gather).  The rank's whole frame then runs on
// P/N rows.
__global__ void __launch_bounds__(256) k_shell_flags(int P, const float* __restrict__ means3D, const float* __restrict__ vm, float lo, float hi,
                                                     uint32_t* __restrict__ flags) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P) return;
    const float3 p = view_point(vm, make_float3(means3D[3 * idx], means3D[3 * idx + 1], means3D[3 * idx + 2]));
    flags[idx] = in_shell(range_of(p), lo, hi) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_wedge_flags(int P, const float* __restrict__ means3D, const float* __restrict__ scales,
                                                     const float* __restrict__ rotations, float mod, const float* __restrict__ vm, float inv_col_step,
                                                     float inv_tan_step, float col_lo, float col_hi, uint32_t* __restrict__ flags) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P) return;
    const float3 p = view_point(vm, make_float3(means3D[3 * idx], means3D[3 * idx + 1], means3D[3 * idx + 2]));
    flags[idx] = wedge_reaches<true>(p, scales, rotations, idx, mod, {inv_col_step, inv_tan_step}, col_lo, col_hi) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_shell_gather(int P, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offs,
                                                      const float* __restrict__ means3D, const float* __restrict__ colors,
                                                      const float* __restrict__ opacities, const float* __restrict__ scales,
                                                      const float* __restrict__ rotations, int* __restrict__ idx_out,
                                                      float* __restrict__ o_means, float* __restrict__ o_colors, float* __restrict__ o_opac,
                                                      float* __restrict__ o_scales, float* __restrict__ o_rot, uint32_t cap,
                                                      const uint32_t* __restrict__ total, uint32_t* __restrict__ n_valid_out,
                                                      int chunk_rows, int world, float* __restrict__ chunk_counts) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    // the gradient all-to-all's split sizes: selected rows whose index lies in chunk d = [d * chunk_rows, (d + 1) * chunk_rows), straight
    // from the scan (offs[i] = selected rows in front of index i); exact as floats (< 2^24 rows per chunk)
    if (chunk_counts && blockIdx.x == 0 && (int)threadIdx.x < world) {
        const uint32_t t = *total, lim = t < cap ? t : cap;
        auto before = [&](long long i) { const uint32_t v = i >= (long long)P ? t : offs[i]; return v < lim ? v : lim; };
        const long long d = threadIdx.x;
        chunk_counts[d] = (float)(before((d + 1) * chunk_rows) - before(d * chunk_rows));
    }
    // capacity-sized selection (enqueue-only rank frames): rows past `cap` are dropped, and the two status words say so --
    // [0] rows gathered = min(selected, cap) (what k_preprocess takes as its n_valid), [1] rows selected
    if (n_valid_out && idx == 0) { const uint32_t t = *total; n_valid_out[0] = t < cap ? t : cap; n_valid_out[1] = t; }
    if (idx >= P || flags[idx] == 0u) return;
    const size_t c = offs[idx];
    if (c >= (size_t)cap) return;
    idx_out[c] = idx;
    for (int k = 0; k < 3; k++) { o_means[3 * c + k] = means3D[3 * (size_t)idx + k]; o_scales[3 * c + k] = scales[3 * (size_t)idx + k]; }
    o_colors[2 * c] = colors[2 * (size_t)idx]; o_colors[2 * c + 1] = colors[2 * (size_t)idx + 1];
    o_opac[c] = opacities[idx];
    reinterpret_cast<float4*>(o_rot)[c] = reinterpret_cast<const float4*>(rotations)[idx];
}

extern "C" size_t lidargs_shell_select_scratch_bytes(int P) {
    const size_t n = P > 0 ? (size_t)P : 1;
    return sizeof(uint32_t) * (2 * n + scan_scratch_words(n) + 64) + 256;
}

// The first steps of a two-step or an enqueue-only selection, either cut: check the scratch (`too_small`: the caller's message), carve
// flags / offsets / total / scan scratch out of it, run the cut's flags launch (`launch_flags(flags)`), then the exclusive scan.
struct SelectScan { uint32_t* flags; uint32_t* offs; uint32_t* total; };
template <class LaunchFlags>
static int select_scan(int P, char* scratch, size_t scratch_bytes, const char* too_small, hipStream_t stream, SelectScan& s, LaunchFlags launch_flags) {
    if (scratch_bytes < lidargs_shell_select_scratch_bytes(P)) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, too_small);
    Carver c(scratch);
    s.flags = c.take<uint32_t>((size_t)P);
    s.offs = c.take<uint32_t>((size_t)P);
    s.total = c.take<uint32_t>(64);
    uint32_t* scan_scratch = c.take<uint32_t>(scan_scratch_words((size_t)P));
    launch_flags(s.flags);
    launch_exclusive_scan(s.flags, s.offs, (size_t)P, s.total, scan_scratch, stream);
    return 0;
}

// the count step: the scan, then the one host read of its total
template <class LaunchFlags>
static int select_count(int P, char* scratch, size_t scratch_bytes, const char* too_small, hipStream_t stream, LaunchFlags launch_flags) {
    SelectScan s;
    if (const int rc = select_scan(P, scratch, scratch_bytes, too_small, stream, s, launch_flags)) return rc;
    uint32_t total_h = 0;
    SH_HIP((hipError_t)api_read_words_zero_behind(s.total, 1, &total_h, nullptr, 0, stream));
    return (int)total_h;
}

// Enqueue-only selections (no host read): flags + scan as above, then the gather into CAPACITY rows.  idx_out's tail is filled with
// 0x7F7F7F7F (above every index: the array stays ascending, and every consumer skips indices >= P); n_valid_dev[0] = rows gathered =
// min(selected, capacity), [1] = rows selected; both words go to status_host (pinned, optional) behind the launches.
template <class LaunchFlags>
static int select_enqueue(int P, const float* means3D, const float* colors, const float* opacities, const float* scales, const float* rotations,
                   int capacity, int* idx_out, float* out_means3D, float* out_colors, float* out_opacities, float* out_scales, float* out_rotations,
                   unsigned* n_valid_dev, unsigned* status_host, char* scratch, size_t scratch_bytes, const char* too_small, int chunk_rows,
                   int world, float* chunk_counts, hipStream_t stream, LaunchFlags launch_flags) {
    SelectScan s;
    if (const int rc = select_scan(P, scratch, scratch_bytes, too_small, stream, s, launch_flags)) return rc;
    if (chunk_counts && (chunk_rows <= 0 || world <= 0 || world > 256)) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "select (enqueue-only): chunk counts need chunk_rows > 0 and 1 <= world <= 256");
    SH_HIP(hipMemsetAsync(idx_out, 0x7F, sizeof(int) * (size_t)capacity, stream));
    hipLaunchKernelGGL(k_shell_gather, dim3((P + 255) / 256), dim3(256), 0, stream, P, s.flags, s.offs, means3D, colors, opacities, scales, rotations, idx_out,
                       out_means3D, out_colors, out_opacities, out_scales, out_rotations, (uint32_t)capacity, s.total, n_valid_dev, chunk_rows, world,
                       chunk_counts);
    if (status_host) SH_HIP(hipMemcpyAsync(status_host, n_valid_dev, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    return api_check_launch(stream, 0, "select gather (enqueue-only)");
}

extern "C" int lidargs_shell_select_count(int P, const float* means3D, const float* viewmatrix, float shell_lo, float shell_hi, char* scratch,
                                          size_t scratch_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_select: P < 0");
    if (P == 0) return 0;
    if (!means3D || !viewmatrix || !scratch) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_select: NULL pointer");
    return select_count(P, scratch, scratch_bytes, "shell_select: scratch too small", stream, [&](uint32_t* flags) {
        hipLaunchKernelGGL(k_shell_flags, dim3((P + 255) / 256), dim3(256), 0, stream, P, means3D, viewmatrix, shell_lo, shell_hi, flags);
    });
}

extern "C" int lidargs_wedge_select_count(int P, const float* means3D, const float* scales, const float* rotations, float scale_modifier,
                                          const float* viewmatrix, int width, int col_lo, int col_hi, char* scratch, size_t scratch_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || width <= 0 || col_lo < 0 || col_hi <= col_lo) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_select: bad sizes");
    if (P == 0) return 0;
    if (!means3D || !viewmatrix || !scratch) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_select: NULL pointer");
    return select_count(P, scratch, scratch_bytes, "wedge_select: scratch too small", stream, [&](uint32_t* flags) {
        const WedgeSteps st = wedge_steps(width);
        hipLaunchKernelGGL(k_wedge_flags, dim3((P + 255) / 256), dim3(256), 0, stream, P, means3D, scales, rotations, scale_modifier, viewmatrix,
                           st.inv_col_step, st.inv_tan_step, (float)col_lo, (float)col_hi, flags);
    });
}

extern "C" int lidargs_shell_select_gather(int P, const float* means3D, const float* colors, const float* opacities, const float* scales,
                                           const float* rotations, int* idx_out, float* out_means3D, float* out_colors, float* out_opacities,
                                           float* out_scales, float* out_rotations, char* scratch, size_t scratch_bytes, int chunk_rows, int world,
                                           float* chunk_counts, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_select: P < 0");
    if (chunk_counts && (chunk_rows <= 0 || world <= 0 || world > 256)) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_select: chunk counts need chunk_rows > 0 and 1 <= world <= 256");
    if (P == 0) {
        if (chunk_counts) SH_HIP(hipMemsetAsync(chunk_counts, 0, sizeof(float) * (size_t)world, stream));
        return 0;
    }
    if (!means3D || !colors || !opacities || !scales || !rotations || !idx_out || !out_means3D || !out_colors || !out_opacities ||
        !out_scales || !out_rotations || !scratch)
        return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_select: NULL pointer");
    if (scratch_bytes < lidargs_shell_select_scratch_bytes(P)) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_select: scratch too small");
    Carver c(scratch);
    uint32_t* flags = c.take<uint32_t>((size_t)P);
    uint32_t* offs = c.take<uint32_t>((size_t)P);
    uint32_t* total = c.take<uint32_t>(64);                            // (left there by the count step)
    hipLaunchKernelGGL(k_shell_gather, dim3((P + 255) / 256), dim3(256), 0, stream, P, flags, offs, means3D, colors, opacities, scales, rotations, idx_out,
                       out_means3D, out_colors, out_opacities, out_scales, out_rotations, 0xFFFFFFFFu, total, (uint32_t*)nullptr, chunk_rows, world,
                       chunk_counts);
    return api_check_launch(stream, 0, "shell select gather");
}

// both steps in one call, into P-row arrays
extern "C" int lidargs_shell_select(int P, const float* means3D, const float* colors, const float* opacities, const float* scales, const float* rotations,
                                    const float* viewmatrix, float shell_lo, float shell_hi, int* idx_out, float* out_means3D, float* out_colors,
                                    float* out_opacities, float* out_scales, float* out_rotations, char* scratch, size_t scratch_bytes, void* stream_) {
    const int M = lidargs_shell_select_count(P, means3D, viewmatrix, shell_lo, shell_hi, scratch, scratch_bytes, stream_);
    if (M <= 0) return M;
    const int rc = lidargs_shell_select_gather(P, means3D, colors, opacities, scales, rotations, idx_out, out_means3D, out_colors, out_opacities,
                                               out_scales, out_rotations, scratch, scratch_bytes, 0, 0, nullptr, stream_);
    return rc < 0 ? rc : M;
}

extern "C" int lidargs_shell_select_enqueue(int P, const float* means3D, const float* colors, const float* opacities, const float* scales,
                                            const float* rotations, const float* viewmatrix, float shell_lo, float shell_hi, int capacity, int* idx_out,
                                            float* out_means3D, float* out_colors, float* out_opacities, float* out_scales, float* out_rotations,
                                            unsigned* n_valid_dev, unsigned* status_host, char* scratch, size_t scratch_bytes, int chunk_rows, int world,
                                            float* chunk_counts, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P <= 0 || capacity <= 0) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_select_enqueue: P and capacity must be positive");
    if (!means3D || !colors || !opacities || !scales || !rotations || !viewmatrix || !idx_out || !out_means3D || !out_colors || !out_opacities ||
        !out_scales || !out_rotations || !n_valid_dev || !scratch)
        return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_select_enqueue: NULL pointer");
    return select_enqueue(P, means3D, colors, opacities, scales, rotations, capacity, idx_out, out_means3D, out_colors, out_opacities, out_scales,
                          out_rotations, n_valid_dev, status_host, scratch, scratch_bytes, "shell_select_enqueue: scratch too small", chunk_rows,
                          world, chunk_counts, stream, [&](uint32_t* flags) {
                              hipLaunchKernelGGL(k_shell_flags, dim3((P + 255) / 256), dim3(256), 0, stream, P, means3D, viewmatrix, shell_lo, shell_hi, flags);
                          });
}

extern "C" int lidargs_wedge_select_enqueue(int P, const float* means3D, const float* colors, const float* opacities, const float* scales,
                                            const float* rotations, float scale_modifier, const float* viewmatrix, int width, int col_lo, int col_hi,
                                            int capacity, int* idx_out, float* out_means3D, float* out_colors, float* out_opacities, float* out_scales,
                                            float* out_rotations, unsigned* n_valid_dev, unsigned* status_host, char* scratch, size_t scratch_bytes,
                                            int chunk_rows, int world, float* chunk_counts, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P <= 0 || capacity <= 0 || width <= 0 || col_lo < 0 || col_hi <= col_lo) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_select_enqueue: bad sizes");
    if (!means3D || !colors || !opacities || !scales || !rotations || !viewmatrix || !idx_out || !out_means3D || !out_colors || !out_opacities ||
        !out_scales || !out_rotations || !n_valid_dev || !scratch)
        return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_select_enqueue: NULL pointer");
    return select_enqueue(P, means3D, colors, opacities, scales, rotations, capacity, idx_out, out_means3D, out_colors, out_opacities, out_scales,
                          out_rotations, n_valid_dev, status_host, scratch, scratch_bytes, "wedge_select_enqueue: scratch too small", chunk_rows,
                          world, chunk_counts, stream, [&](uint32_t* flags) {
                              const WedgeSteps st = wedge_steps(width);
                              hipLaunchKernelGGL(k_wedge_flags, dim3((P + 255) / 256), dim3(256), 0, stream, P, means3D, scales, rotations, scale_modifier,
                                                 viewmatrix, st.inv_col_step, st.inv_tan_step, (float)col_lo, (float)col_hi, flags);
                          });
}

// ------------------------------------------------------------------------------------------------
// The selection in ONE launch (round 6, round-5 verdict item 4a; NOT the default: bit-identical to the two-step form,
// tests/test_dist_gpu.py, and no faster -- 215-247 us against 88 + 38 + 78 us at 8 M Gaussians, EXPERIMENTS.md).
// flags -> scan (three launches over P) -> gather read every replicated Gaussian's position twice and wrote / read 8 bytes of flags and
// offsets per Gaussian in between: 238 us of an 8 M-Gaussian wedge rank's 0.90-ms frame.  Here a block tests 1024 consecutive
// Gaussians, scans its flags in index order (the selection stays ascending: equal ranges break ties by index), learns the rows in front
// of it by decoupled look-back over the blocks before it (each block publishes its count, then its inclusive prefix, in one 64-bit
// word; blocks take their number from a ticket so that a block only ever waits for blocks that are already running), and writes the
// selected rows itself.  The block that finishes last writes the row counts and the gradient all-to-all's split sizes (lower bounds on
// the ascending index array it can now read).
#define SEL_ITEMS 4
#define SEL_BLOCK (256 * SEL_ITEMS)
struct SelArgs {
    int P; const float* means; const float* colors; const float* opac; const float* scales; const float* rot; const float* vm;
    float lo, hi;                                                      // shell: range in [lo, hi)
    float mod; WedgeSteps steps; float col_lo, col_hi;                 // wedge: the inputs of wedge_reaches
    uint32_t cap; int* idx_out; float* o_means; float* o_colors; float* o_opac; float* o_scales; float* o_rot;
    uint32_t* n_valid_out; int chunk_rows, world; float* chunk_counts;
    unsigned long long* status; uint32_t* ticket;                      // [blocks] (flag << 32 | value), [2]: ticket, finished blocks -- zeroed by the caller
    unsigned blocks;
};
inline size_t select_fused_words(size_t P) { return 2 * ((P + SEL_BLOCK - 1) / SEL_BLOCK) + 8; }      // u32 words of zeroed scratch: status (u64 per block) + ticket + finished
template <bool WEDGE>
__global__ void __launch_bounds__(256) k_select_fused(const SelArgs a) {
    __shared__ uint32_t s_bid, s_cnt[SEL_ITEMS][4], s_base, s_total;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_bid = atomicAdd(a.ticket, 1u);
    __syncthreads();
    const unsigned b = s_bid;
    const size_t base = (size_t)b * SEL_BLOCK;
    const float* __restrict__ vm = a.vm;
    bool f[SEL_ITEMS];
    float3 pw[SEL_ITEMS];
#pragma unroll
    for (int j = 0; j < SEL_ITEMS; j++) {
        const size_t idx = base + (size_t)j * 256 + tid;
        f[j] = false; pw[j] = make_float3(0.f, 0.f, 0.f);
        if (idx < (size_t)a.P) {
            pw[j] = make_float3(a.means[3 * idx], a.means[3 * idx + 1], a.means[3 * idx + 2]);
            const float3 p = view_point(vm, pw[j]);
            if (!WEDGE) f[j] = in_shell(range_of(p), a.lo, a.hi);
            else f[j] = wedge_reaches<false>(p, a.scales, a.rot, idx, a.mod, a.steps, a.col_lo, a.col_hi);
        }
    }
    // flags in index order inside the block: item-major (item j covers indices base + 256 j ..), then wave, then lane
    uint32_t within[SEL_ITEMS];
#pragma unroll
    for (int j = 0; j < SEL_ITEMS; j++) {
        const unsigned long long m = __ballot(f[j]);
        within[j] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[j][w] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    // exclusive offsets of the 4 x SEL_ITEMS (item, wave) cells, in index order, by the first wave (one cell per lane: SEL_ITEMS * 4 <= 64)
    static_assert(SEL_ITEMS * 4 <= 64, "one cell per lane");
    if (w == 0) {
        const uint32_t c = lane < SEL_ITEMS * 4 ? (&s_cnt[0][0])[lane] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o); if (lane >= o) incl += v; }
        if (lane < SEL_ITEMS * 4) (&s_cnt[0][0])[lane] = incl - c;
        if (lane == 63) s_total = incl;
    }
    __syncthreads();
    const uint32_t total = s_total;
    uint32_t off[SEL_ITEMS];
#pragma unroll
    for (int j = 0; j < SEL_ITEMS; j++) off[j] = s_cnt[j][w];
    if (w == 0) {
        // decoupled look-back by one WAVE: lane l reads the word of block p - l; the nearest block that already knows its inclusive prefix ends
        // the walk, the aggregates of the blocks in front of it are added.  (One thread walking word by word waited a full memory round trip
        // per predecessor: 8 k blocks looked back one after the other -- 5 ms for a 0.2-ms job.)
        uint32_t excl = 0;
        if (b > 0) {
            if (lane == 0) __hip_atomic_store(a.status + b, (1ull << 32) | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            long long p = (long long)b - 1;                            // the nearest block not yet accounted for
            for (;;) {
                const long long mine = p - lane;
                unsigned long long v = 2ull << 32;                    // in front of block 0: an inclusive prefix of 0
                if (mine >= 0) v = __hip_atomic_load(a.status + mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long empty = __ballot((v >> 32) == 0ull);
                const unsigned long long pref = __ballot((v >> 32) == 2ull);
                // usable lanes: those nearer than the first empty one; among them the nearest prefix ends the walk
                const int first_empty = empty ? __builtin_ctzll(empty) : 64;
                const int first_pref = pref ? __builtin_ctzll(pref) : 64;
                const int upto = first_pref < first_empty ? first_pref + 1 : first_empty;      // lanes [0, upto) are added
                uint32_t add = lane < upto ? (uint32_t)v : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) add += __shfl_xor(add, o);
                excl += add;
                if (first_pref < first_empty) break;
                p -= upto;
                if (upto == 0) __builtin_amdgcn_s_sleep(2);
            }
        }
        if (lane == 0) {
            __hip_atomic_store(a.status + b, (2ull << 32) | (unsigned long long)(excl + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_base = excl;
        }
    }
    __syncthreads();
    const uint32_t blk = s_base;
#pragma unroll
    for (int j = 0; j < SEL_ITEMS; j++) {
        if (!f[j]) continue;
        const size_t idx = base + (size_t)j * 256 + tid;
        const size_t c = (size_t)blk + off[j] + within[j];
        if (c >= (size_t)a.cap) continue;
        a.idx_out[c] = (int)idx;
        a.o_means[3 * c] = pw[j].x; a.o_means[3 * c + 1] = pw[j].y; a.o_means[3 * c + 2] = pw[j].z;
        for (int k = 0; k < 3; k++) a.o_scales[3 * c + k] = a.scales[3 * idx + k];
        reinterpret_cast<float2*>(a.o_colors)[c] = reinterpret_cast<const float2*>(a.colors)[idx];
        a.o_opac[c] = a.opac[idx];
        reinterpret_cast<float4*>(a.o_rot)[c] = reinterpret_cast<const float4*>(a.rot)[idx];
    }
    // Row counts and the gradient all-to-all's split sizes, without reading another block's rows (no fence anywhere in this launch: a
    // word of the look-back carries its own data, relaxed 64-bit atomics suffice -- with release / acquire every block wrote the L2 back
    // and the 8 k blocks of an 8 M-Gaussian frame went through one after the other, 2.2 ms).  counts[d] = before((d + 1) chunk) - before(d chunk)
    // with before(i) = selected rows with index < i, clamped at the capacity: the block that holds index i adds +before(i) to counts[d - 1]
    // and -before(i) to counts[d] (float atomics on integers < 2^24: exact, any order; zeroed by the caller); the block that holds the last
    // index adds the total.
    const bool last_block = base + SEL_BLOCK >= (size_t)a.P;
    if (a.chunk_counts) {
        for (int d = 1; d < a.world; d++) {
            const long long i_d = (long long)d * a.chunk_rows;
            if (i_d < (long long)base || i_d >= (long long)base + SEL_BLOCK || i_d >= (long long)a.P) continue;     // (block-uniform)
            uint32_t c = 0;
#pragma unroll
            for (int j = 0; j < SEL_ITEMS; j++) c += (f[j] && (long long)(base + (size_t)j * 256 + tid) < i_d) ? 1u : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
            __syncthreads();
            if (lane == 0) s_cnt[0][w] = c;
            __syncthreads();
            if (tid == 0) {
                uint32_t v = blk + s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
                v = v < a.cap ? v : a.cap;
                atomicAdd(a.chunk_counts + d - 1, (float)v); atomicAdd(a.chunk_counts + d, -(float)v);
            }
        }
    }
    if (last_block && tid == 0) {
        const uint32_t t = blk + total, n = t < a.cap ? t : a.cap;
        if (a.n_valid_out) { a.n_valid_out[0] = n; a.n_valid_out[1] = t; }
        if (a.chunk_counts) {
            // boundaries at or behind P see every selected row in front of them
            for (int d = 1; d <= a.world; d++) {
                const long long i_d = (long long)d * a.chunk_rows;
                if (d < a.world && i_d < (long long)a.P) continue;
                atomicAdd(a.chunk_counts + d - 1, (float)n);
                if (d < a.world) atomicAdd(a.chunk_counts + d, -(float)n);
            }
        }
    }
}
// the one-launch selection into `capacity` rows; fill_tail: idx_out's tail = 0x7F7F7F7F (enqueue-only frames: the array stays ascending
// and every consumer skips indices >= P); wait: read the two counts back and return the rows gathered
static int select_fused(bool wedge, SelArgs a, int capacity, unsigned* n_valid_dev, unsigned* status_host, char* scratch, size_t scratch_bytes,
                        bool fill_tail, bool wait, hipStream_t stream) {
    if (a.chunk_counts && (a.chunk_rows <= 0 || a.world <= 0 || a.world > 256)) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "select: chunk counts need chunk_rows > 0 and 1 <= world <= 256");
    if (scratch_bytes < lidargs_shell_select_scratch_bytes(a.P)) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "select: scratch too small");
    Carver c(scratch);
    const size_t words = select_fused_words((size_t)a.P);
    uint32_t* z = c.take<uint32_t>(words + 2);
    a.ticket = z; a.status = reinterpret_cast<unsigned long long*>(z + 2);       // (128-byte aligned base: the 64-bit words are 8-byte aligned)
    a.cap = (uint32_t)capacity; a.n_valid_out = n_valid_dev;
    SH_HIP(hipMemsetAsync(z, 0, sizeof(uint32_t) * (words + 2), stream));
    if (fill_tail) SH_HIP(hipMemsetAsync(a.idx_out, 0x7F, sizeof(int) * (size_t)capacity, stream));
    if (a.chunk_counts) SH_HIP(hipMemsetAsync(a.chunk_counts, 0, sizeof(float) * (size_t)a.world, stream));
    a.blocks = (unsigned)(((size_t)a.P + SEL_BLOCK - 1) / SEL_BLOCK);
    if (wedge) hipLaunchKernelGGL(k_select_fused<true>, dim3(a.blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_select_fused<false>, dim3(a.blocks), dim3(256), 0, stream, a);
    if (status_host) SH_HIP(hipMemcpyAsync(status_host, n_valid_dev, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    const int rc = api_check_launch(stream, 0, "select (one launch)");
    if (rc || !wait) return rc;
    uint32_t h[2] = {0, 0};
    SH_HIP((hipError_t)api_read_words_zero_behind(n_valid_dev, 2, h, nullptr, 0, stream));
    return (int)h[0];
}
static SelArgs sel_args(int P, const float* means3D, const float* colors, const float* opacities, const float* scales, const float* rotations, const float* viewmatrix,
                     int* idx_out, float* out_means3D, float* out_colors, float* out_opacities, float* out_scales, float* out_rotations, int chunk_rows, int world,
                     float* chunk_counts) {
    SelArgs a = SelArgs();
    a.P = P; a.means = means3D; a.colors = colors; a.opac = opacities; a.scales = scales; a.rot = rotations; a.vm = viewmatrix;
    a.idx_out = idx_out; a.o_means = out_means3D; a.o_colors = out_colors; a.o_opac = out_opacities; a.o_scales = out_scales; a.o_rot = out_rotations;
    a.chunk_rows = chunk_rows; a.world = world; a.chunk_counts = chunk_counts;
    return a;
}
// the same into P-row arrays, with the one host read the two-step form makes as well; returns the rows gathered M
extern "C" int lidargs_shell_select_sync(int P, const float* means3D, const float* colors, const float* opacities, const float* scales, const float* rotations,
                                         const float* viewmatrix, float shell_lo, float shell_hi, int capacity, int* idx_out, float* out_means3D, float* out_colors,
                                         float* out_opacities, float* out_scales, float* out_rotations, unsigned* n_valid_dev, char* scratch, size_t scratch_bytes,
                                         int chunk_rows, int world, float* chunk_counts, void* stream_) {
    if (P < 0 || capacity < 0) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_select_sync: bad sizes");
    if (P == 0 || capacity == 0) {
        if (chunk_counts && world > 0) SH_HIP(hipMemsetAsync(chunk_counts, 0, sizeof(float) * (size_t)world, (hipStream_t)stream_));
        return 0;
    }
    if (!means3D || !colors || !opacities || !scales || !rotations || !viewmatrix || !idx_out || !out_means3D || !out_colors || !out_opacities ||
        !out_scales || !out_rotations || !n_valid_dev || !scratch)
        return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_select_sync: NULL pointer");
    SelArgs a = sel_args(P, means3D, colors, opacities, scales, rotations, viewmatrix, idx_out, out_means3D, out_colors, out_opacities, out_scales, out_rotations,
                             chunk_rows, world, chunk_counts);
    a.lo = shell_lo; a.hi = shell_hi;
    return select_fused(false, a, capacity, n_valid_dev, nullptr, scratch, scratch_bytes, false, true, (hipStream_t)stream_);
}
extern "C" int lidargs_wedge_select_sync(int P, const float* means3D, const float* colors, const float* opacities, const float* scales, const float* rotations,
                                         float scale_modifier, const float* viewmatrix, int width, int col_lo, int col_hi, int capacity, int* idx_out, float* out_means3D,
                                         float* out_colors, float* out_opacities, float* out_scales, float* out_rotations, unsigned* n_valid_dev, char* scratch,
                                         size_t scratch_bytes, int chunk_rows, int world, float* chunk_counts, void* stream_) {
    if (P < 0 || capacity < 0 || width <= 0 || col_lo < 0 || col_hi <= col_lo) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_select_sync: bad sizes");
    if (P == 0 || capacity == 0) {
        if (chunk_counts && world > 0) SH_HIP(hipMemsetAsync(chunk_counts, 0, sizeof(float) * (size_t)world, (hipStream_t)stream_));
        return 0;
    }
    if (!means3D || !colors || !opacities || !scales || !rotations || !viewmatrix || !idx_out || !out_means3D || !out_colors || !out_opacities ||
        !out_scales || !out_rotations || !n_valid_dev || !scratch)
        return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_select_sync: NULL pointer");
    SelArgs a = sel_args(P, means3D, colors, opacities, scales, rotations, viewmatrix, idx_out, out_means3D, out_colors, out_opacities, out_scales, out_rotations,
                             chunk_rows, world, chunk_counts);
    a.mod = scale_modifier; a.steps = wedge_steps(width); a.col_lo = (float)col_lo; a.col_hi = (float)col_hi;
    return select_fused(true, a, capacity, n_valid_dev, nullptr, scratch, scratch_bytes, false, true, (hipStream_t)stream_);
}

// ------------------------------------------------------------------------------------------------
// Gradient rows of a range shell (lidargs_dist step 6): the six returned gradients of the shell's M Gaussians + their global
// index as one [M, 18] row block (what the all-to-all ships), and back: rows scattered by index into a dense [P, 17] block.
// One launch each instead of a concatenate, casts, an index_copy and their temporaries.
__global__ void __launch_bounds__(256) k_shell_pack_rows(int M, const float* __restrict__ g_m3, const float* __restrict__ g_m2,
                                                         const float* __restrict__ g_col, const float* __restrict__ g_op,
                                                         const float* __restrict__ g_sc, const float* __restrict__ g_rot,
                                                         const int* __restrict__ idx, float* __restrict__ rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    float* r = rows + 18 * (size_t)i;
    r[0] = g_m3[3 * (size_t)i]; r[1] = g_m3[3 * (size_t)i + 1]; r[2] = g_m3[3 * (size_t)i + 2];
    const float4 m2 = reinterpret_cast<const float4*>(g_m2)[i];
    r[3] = m2.x; r[4] = m2.y; r[5] = m2.z; r[6] = m2.w;
    const float2 c = reinterpret_cast<const float2*>(g_col)[i];
    r[7] = c.x; r[8] = c.y;
    r[9] = g_op[i];
    r[10] = g_sc[3 * (size_t)i]; r[11] = g_sc[3 * (size_t)i + 1]; r[12] = g_sc[3 * (size_t)i + 2];
    const float4 q = reinterpret_cast<const float4*>(g_rot)[i];
    r[13] = q.x; r[14] = q.y; r[15] = q.z; r[16] = q.w;
    r[17] = __int_as_float(idx[i]);                                    // the index travels as a bit pattern
}
extern "C" int lidargs_shell_pack_grad_rows(int M, const float* dL_dmeans3D, const float* dL_dmeans2D, const float* dL_dcolors, const float* dL_dopacity,
                                            const float* dL_dscales, const float* dL_drotations, const int* idx, float* rows, void* stream) {
    if (M < 0) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_pack_grad_rows: M < 0");
    if (M == 0) return 0;
    if (!dL_dmeans3D || !dL_dmeans2D || !dL_dcolors || !dL_dopacity || !dL_dscales || !dL_drotations || !idx || !rows)
        return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_pack_grad_rows: NULL pointer");
    hipLaunchKernelGGL(k_shell_pack_rows, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, M, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dscales,
                       dL_drotations, idx, rows);
    return api_check_launch((hipStream_t)stream, 0, "shell pack rows");
}
// Round 6: only the rows that carry a gradient travel.  A frame blends a fraction of the Gaussians a rank preprocesses (cfg4: 10 k of 8 M;
// cfg3: a fifth) and every other row of the exchange is 72 bytes of zeros -- packed, shipped over xGMI, read and skipped.  Two launches
// around one host read (the all-to-all's split sizes are host numbers anyway): count the rows with any non-zero gradient per destination
// chunk, then write exactly those, grouped by destination (any order inside a group: the receiver scatters by index).
__device__ __forceinline__ bool shell_row_live(const float* __restrict__ g_m3, const float* __restrict__ g_m2, const float* __restrict__ g_col, const float* __restrict__ g_op,
                                               const float* __restrict__ g_sc, const float* __restrict__ g_rot, size_t i, float* r) {
    r[0] = g_m3[3 * i]; r[1] = g_m3[3 * i + 1]; r[2] = g_m3[3 * i + 2];
    const float4 m2 = reinterpret_cast<const float4*>(g_m2)[i];
    r[3] = m2.x; r[4] = m2.y; r[5] = m2.z; r[6] = m2.w;
    const float2 c = reinterpret_cast<const float2*>(g_col)[i];
    r[7] = c.x; r[8] = c.y;
    r[9] = g_op[i];
    r[10] = g_sc[3 * i]; r[11] = g_sc[3 * i + 1]; r[12] = g_sc[3 * i + 2];
    const float4 q = reinterpret_cast<const float4*>(g_rot)[i];
    r[13] = q.x; r[14] = q.y; r[15] = q.z; r[16] = q.w;
    bool live = false;
#pragma unroll
    for (int k = 0; k < 17; k++) live = live || (r[k] != 0.f);          // (a NaN is != 0: it travels)
    return live;
}
// WRITE = false: counts[d] += live rows bound for chunk d.  WRITE = true: rows_out[prefix(counts)[d] + cursor[d]++] = the row.
template <bool WRITE>
__global__ void __launch_bounds__(256) k_shell_pack_rows_live(int M, const float* __restrict__ g_m3, const float* __restrict__ g_m2, const float* __restrict__ g_col,
                                                              const float* __restrict__ g_op, const float* __restrict__ g_sc, const float* __restrict__ g_rot,
                                                              const int* __restrict__ idx, int P, int chunk_rows, int world, uint32_t* __restrict__ counts,
                                                              uint32_t* __restrict__ cursor, float* __restrict__ rows_out) {
    __shared__ uint32_t s_base[256];
    if (WRITE) {
        // exclusive prefix of the counts (world <= 256): where each destination's group starts
        const int t = threadIdx.x;
        uint32_t v = t < world ? counts[t] : 0u, incl = v;
        const int lane = t & 63;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o); if (lane >= o) incl += u; }
        __shared__ uint32_t s_w[4];
        if (lane == 63) s_w[t >> 6] = incl;
        __syncthreads();
        uint32_t off = 0;
        for (int q = 0; q < (t >> 6); q++) off += s_w[q];
        s_base[t] = off + incl - v;
        __syncthreads();
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    float r[17];
    int g = -1;
    bool live = false;
    if (i < M) {
        g = idx[i];
        if (g >= 0 && g < P) live = shell_row_live(g_m3, g_m2, g_col, g_op, g_sc, g_rot, (size_t)i, r);
    }
    const int d = live ? min(g / chunk_rows, world - 1) : -1;
    // wave-aggregated per destination: the rows of a wave are index-ascending, so it sees one destination, rarely two
    unsigned long long todo = __ballot(live);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const int dl = __shfl(d, leader);
        const unsigned long long same = __ballot(live && d == dl);
        uint32_t pos = 0;
        if (lane == leader) pos = atomicAdd((WRITE ? cursor : counts) + dl, (uint32_t)__builtin_popcountll(same));
        pos = __shfl(pos, leader);
        if (WRITE && live && d == dl) {
            float* o = rows_out + 18 * ((size_t)s_base[dl] + pos + (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1ull)));
#pragma unroll
            for (int k = 0; k < 17; k++) o[k] = r[k];
            o[17] = __int_as_float(g);
        }
        todo &= ~same;
    }
}
// Step 1 counts them per
// destination chunk into counts_dev u32[world] (zeroed here) and copies the counts to counts_host (waits: the all-to-all's split sizes are
// host numbers); step 2 writes exactly sum(counts) rows of 18 floats, grouped by destination in ascending chunk order (cursor u32[world] is
// scratch, zeroed here).  Returns the number of live rows (step 1) / 0 (step 2).
extern "C" int lidargs_shell_pack_grad_rows_live_count(int M, const float* dL_dmeans3D, const float* dL_dmeans2D, const float* dL_dcolors, const float* dL_dopacity,
                                                       const float* dL_dscales, const float* dL_drotations, const int* idx, int P, int chunk_rows, int world,
                                                       unsigned* counts_dev, unsigned* counts_host, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (M < 0 || P < 0 || chunk_rows <= 0 || world <= 0 || world > 256 || !counts_dev) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_pack_grad_rows_live_count: bad arguments");
    SH_HIP(hipMemsetAsync(counts_dev, 0, sizeof(unsigned) * (size_t)world, stream));
    if (M > 0) {
        if (!dL_dmeans3D || !dL_dmeans2D || !dL_dcolors || !dL_dopacity || !dL_dscales || !dL_drotations || !idx)
            return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_pack_grad_rows_live_count: NULL pointer");
        hipLaunchKernelGGL(k_shell_pack_rows_live<false>, dim3((M + 255) / 256), dim3(256), 0, stream, M, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dscales,
                           dL_drotations, idx, P, chunk_rows, world, counts_dev, (uint32_t*)nullptr, (float*)nullptr);
    }
    if (!counts_host) return api_check_launch(stream, 0, "shell pack rows (live count)");      // the counts stay on the device (the caller gathers every rank's and reads them once)
    SH_HIP((hipError_t)api_read_words_zero_behind(counts_dev, world, counts_host, nullptr, 0, stream));
    long long tot = 0;
    for (int d = 0; d < world; d++) tot += counts_host[d];
    return (int)tot;
}
extern "C" int lidargs_shell_pack_grad_rows_live(int M, const float* dL_dmeans3D, const float* dL_dmeans2D, const float* dL_dcolors, const float* dL_dopacity,
                                                 const float* dL_dscales, const float* dL_drotations, const int* idx, int P, int chunk_rows, int world,
                                                 unsigned* counts_dev, unsigned* cursor_dev, float* rows, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (M < 0 || P < 0 || chunk_rows <= 0 || world <= 0 || world > 256 || !counts_dev || !cursor_dev) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_pack_grad_rows_live: bad arguments");
    if (M == 0) return 0;
    if (!dL_dmeans3D || !dL_dmeans2D || !dL_dcolors || !dL_dopacity || !dL_dscales || !dL_drotations || !idx || !rows)
        return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_pack_grad_rows_live: NULL pointer");
    SH_HIP(hipMemsetAsync(cursor_dev, 0, sizeof(unsigned) * (size_t)world, stream));
    hipLaunchKernelGGL(k_shell_pack_rows_live<true>, dim3((M + 255) / 256), dim3(256), 0, stream, M, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dscales,
                       dL_drotations, idx, P, chunk_rows, world, counts_dev, cursor_dev, rows);
    return api_check_launch(stream, 0, "shell pack rows (live)");
}
// blocked != 0: dense is six contiguous blocks [P,3][P,4][P,2][P,1][P,3][P,4] (what autograd takes without a strided copy each)
// base (round 6, the "shard" gradient mode): `dense` holds the rows [base, base + P) of the index space only -- a rank's own chunk
__global__ void __launch_bounds__(256) k_shell_unpack_rows(int n, const float* __restrict__ rows, int P, float* __restrict__ dense, int blocked, int base) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = rows + 18 * (size_t)i;
    const int g = __float_as_int(r[17]) - base;
    if (g < 0 || g >= P) return;
    if (!blocked) {
        float* d = dense + 17 * (size_t)g;
#pragma unroll
        for (int k = 0; k < 17; k++) d[k] = r[k];
        return;
    }
    const size_t Ps = (size_t)P, gs = (size_t)g;
    float* d = dense + 3 * gs;            d[0] = r[0]; d[1] = r[1]; d[2] = r[2];
    d = dense + 3 * Ps + 4 * gs;          d[0] = r[3]; d[1] = r[4]; d[2] = r[5]; d[3] = r[6];
    d = dense + 7 * Ps + 2 * gs;          d[0] = r[7]; d[1] = r[8];
    dense[9 * Ps + gs] = r[9];
    d = dense + 10 * Ps + 3 * gs;         d[0] = r[10]; d[1] = r[11]; d[2] = r[12];
    d = dense + 13 * Ps + 4 * gs;         d[0] = r[13]; d[1] = r[14]; d[2] = r[15]; d[3] = r[16];
}
// Column wedges: a Gaussian whose rect straddles a wedge boundary has gradient rows on two (or more) ranks; the owner ADDS them.
// dense = six contiguous blocks (blocked layout), zeroed by the caller.
__global__ void __launch_bounds__(256) k_shell_unpack_rows_add(int n, const float* __restrict__ rows, int P, float* __restrict__ dense, int base) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = rows + 18 * (size_t)i;
    const int g = __float_as_int(r[17]) - base;
    if (g < 0 || g >= P) return;
    const size_t Ps = (size_t)P, gs = (size_t)g;
    const int off[6] = {0, 3, 7, 9, 10, 13}, wid[6] = {3, 4, 2, 1, 3, 4};
#pragma unroll
    for (int b = 0; b < 6; b++)
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < wid[b]) {
                const float v = r[off[b] + k];
                if (v != 0.f) atomicAdd(dense + off[b] * Ps + wid[b] * gs + k, v);
            }
}
extern "C" int lidargs_shell_unpack_grad_rows(int n, const float* rows, int P, float* dense, int blocked, void* stream) {
    if (n < 0 || P < 0) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_unpack_grad_rows: bad sizes");
    if (P == 0) return 0;
    if (!dense || (n > 0 && !rows)) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_unpack_grad_rows: NULL pointer");
    SH_HIP(hipMemsetAsync(dense, 0, sizeof(float) * 17 * (size_t)P, (hipStream_t)stream));
    if (n) hipLaunchKernelGGL(k_shell_unpack_rows, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, rows, P, dense, blocked, 0);
    return api_check_launch((hipStream_t)stream, 0, "shell unpack rows");
}
extern "C" int lidargs_wedge_unpack_grad_rows_add(int n, const float* rows, int P, float* dense, void* stream) {
    if (n < 0 || P < 0) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_unpack_grad_rows_add: bad sizes");
    if (P == 0) return 0;
    if (!dense || (n > 0 && !rows)) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_unpack_grad_rows_add: NULL pointer");
    SH_HIP(hipMemsetAsync(dense, 0, sizeof(float) * 17 * (size_t)P, (hipStream_t)stream));
    if (n) hipLaunchKernelGGL(k_shell_unpack_rows_add, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, rows, P, dense, 0);
    return api_check_launch((hipStream_t)stream, 0, "wedge unpack rows");
}
// Round 6, gradient mode "shard": the rows a rank received for its OWN index chunk [base, base + chunk_rows), unpacked into a
// [17][chunk_rows] block (six contiguous gradient blocks of chunk_rows rows each) -- no dense [P, 17] block is zero-filled or scattered into
// (544 MB + 20 M scattered words per frame at 8 M Gaussians).  add != 0: rows of equal index are added (column wedges).
extern "C" int lidargs_shell_unpack_grad_rows_chunk(int n, const float* rows, int base, int chunk_rows, float* dense, int add, void* stream) {
    if (n < 0 || base < 0 || chunk_rows < 0) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_unpack_grad_rows_chunk: bad sizes");
    if (chunk_rows == 0) return 0;
    if (!dense || (n > 0 && !rows)) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_unpack_grad_rows_chunk: NULL pointer");
    SH_HIP(hipMemsetAsync(dense, 0, sizeof(float) * 17 * (size_t)chunk_rows, (hipStream_t)stream));
    if (n) {
        if (add) hipLaunchKernelGGL(k_shell_unpack_rows_add, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, rows, chunk_rows, dense, base);
        else hipLaunchKernelGGL(k_shell_unpack_rows, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, rows, chunk_rows, dense, 1, base);
    }
    return api_check_launch((hipStream_t)stream, 0, "shell unpack rows (chunk)");
}
// counts[d] = #(idx in [d * chunk, (d + 1) * chunk)), idx ascending: the split sizes of the gradient all-to-all
__global__ void __launch_bounds__(64) k_shell_chunk_counts(int M, const int* __restrict__ idx, int chunk, int world, float* __restrict__ counts) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= world) return;
    auto lower = [&](long long v) { int lo = 0, hi = M; while (lo < hi) { const int md = (lo + hi) >> 1; if ((long long)idx[md] < v) lo = md + 1; else hi = md; } return lo; };
    counts[d] = (float)(lower((long long)(d + 1) * chunk) - lower((long long)d * chunk));
}
extern "C" int lidargs_shell_chunk_counts(int M, const int* idx, int chunk_rows, int world, float* counts, void* stream) {
    if (M < 0 || chunk_rows <= 0 || world <= 0 || !counts || (M > 0 && !idx)) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_chunk_counts: bad arguments");
    hipLaunchKernelGGL(k_shell_chunk_counts, dim3((world + 63) / 64), dim3(64), 0, (hipStream_t)stream, M, idx, chunk_rows, world, counts);
    return api_check_launch((hipStream_t)stream, 0, "shell chunk counts");
}
__global__ void __launch_bounds__(256) k_shell_scatter_i32(int M, const int* __restrict__ idx, const int* __restrict__ src, int P, int* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int g = idx[i];
    if (g >= 0 && g < P) dst[g] = src[i];
}
extern "C" int lidargs_shell_scatter_radii(int M, const int* idx, const int* radii_shell, int P, int* radii, void* stream) {
    if (M < 0 || P < 0) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_scatter_radii: bad sizes");
    if (P == 0) return 0;
    if (!radii || (M > 0 && (!idx || !radii_shell))) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_scatter_radii: NULL pointer");
    SH_HIP(hipMemsetAsync(radii, 0, sizeof(int) * (size_t)P, (hipStream_t)stream));
    if (M) hipLaunchKernelGGL(k_shell_scatter_i32, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, M, idx, radii_shell, P, radii);
    return api_check_launch((hipStream_t)stream, 0, "shell scatter radii");
}

#pragma clang fp contract(fast)

// ------------------------------------------------------------------------------------------------
// Per-pixel folds over the G range shells, one launch each instead of a dozen
// elementwise framework ops on a 0.2 ms critical path.
__global__ void __launch_bounds__(256) k_shell_transmittance(int G, int rank, int N, size_t row_stride, const float* __restrict__ all_T, float* __restrict__ T_in) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float T = 1.f;
    for (int g = 0; g < rank && g < G; g++) T *= all_T[(size_t)g * row_stride + i];
    T_in[i] = T;
}
extern "C" int lidargs_shell_transmittance(int G, int rank, int N, size_t row_stride, const float* all_T, float* T_in, void* stream_) {
    if (G < 1 || rank < 0 || rank >= G || N < 0 || row_stride < (size_t)N || !all_T || !T_in) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_transmittance: bad argument");
    if (N) hipLaunchKernelGGL(k_shell_transmittance, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream_, G, rank, N, row_stride, all_T, T_in);
    return 0;
}

// planes[g] = (C0, C1, D, T_end, T_hand) of shell g.  The walk stopped in the first shell whose hand-over value fell
// below the reference's 1e-4 threshold; T_final is that shell's T_end (the last shell's if none stopped).
__global__ void __launch_bounds__(256) k_shell_compose(int G, int rank, int N, const float* __restrict__ planes, const float* __restrict__ bg,
                                                       float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ out_occ,
                                                       float* __restrict__ T_final, float* __restrict__ behind) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float c0 = 0.f, c1 = 0.f, d = 0.f, b0 = 0.f, b1 = 0.f, bd = 0.f, Tf = 1.f;
    bool stopped = false;
    for (int g = 0; g < G; g++) {
        const float* p = planes + (size_t)g * 5 * N + i;
        const float pc0 = p[0], pc1 = p[(size_t)N], pd = p[2 * (size_t)N];
        c0 += pc0; c1 += pc1; d += pd;
        if (g > rank) { b0 += pc0; b1 += pc1; bd += pd; }
        if (!stopped) { Tf = p[3 * (size_t)N]; stopped = p[4 * (size_t)N] < 0.0001f; }
    }
    const float g0 = bg ? bg[0] : 0.f, g1 = bg ? bg[1] : 0.f;
    out_color[i] = c0 + Tf * g0; out_color[(size_t)N + i] = c1 + Tf * g1;
    out_depth[i] = d; out_occ[i] = 1.f - Tf; T_final[i] = Tf;
    behind[i] = b0; behind[(size_t)N + i] = b1; behind[2 * (size_t)N + i] = bd;
}
extern "C" int lidargs_shell_compose(int G, int rank, int N, const float* planes, const float* background, float* out_color, float* out_depth,
                                     float* out_occ, float* T_final, float* behind, void* stream_) {
    if (G < 1 || rank < 0 || rank >= G || N < 0 || !planes || !out_color || !out_depth || !out_occ || !T_final || !behind)
        return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "shell_compose: bad argument");
    if (N) hipLaunchKernelGGL(k_shell_compose, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream_, G, rank, N, planes, background, out_color, out_depth, out_occ, T_final,
                              behind);
    return 0;
}

// Column wedges: a rank's own pixel columns [c0, c1) of the four image planes (colour 0/1, depth, occupancy) as one dense
// [4][H][wmax] block (what the image all-gather ships; columns >= c1 - c0 are padding), and back: G such blocks -> full planes.
__global__ void __launch_bounds__(256) k_wedge_pack_columns(int H, int W, int c0, int c1, int wmax, const float* __restrict__ color,
                                                            const float* __restrict__ depth, const float* __restrict__ occ, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = 4 * H * wmax;
    if (i >= n) return;
    const int x = i % wmax, y = (i / wmax) % H, pl = i / (wmax * H);
    const int col = c0 + x;
    float v = 0.f;
    if (col < c1) {
        const size_t pix = (size_t)y * W + col;
        v = pl < 2 ? color[(size_t)pl * H * W + pix] : (pl == 2 ? depth[pix] : occ[pix]);
    }
    out[i] = v;
}
extern "C" int lidargs_wedge_pack_columns(int height, int width, int col_lo, int col_hi, int wmax, const float* color, const float* depth, const float* occ,
                                          float* out, void* stream) {
    if (height <= 0 || width <= 0 || col_lo < 0 || col_hi <= col_lo || col_hi > width || wmax < col_hi - col_lo || !color || !depth || !occ || !out)
        return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_pack_columns: bad argument");
    const int n = 4 * height * wmax;
    hipLaunchKernelGGL(k_wedge_pack_columns, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, height, width, col_lo, col_hi, wmax, color, depth, occ, out);
    return api_check_launch((hipStream_t)stream, 0, "wedge pack columns");
}
struct WedgeEdges { int e[65]; };
__global__ void __launch_bounds__(256) k_wedge_unpack_columns(int G, int H, int W, int wmax, size_t stride, WedgeEdges ed, const float* __restrict__ blocks,
                                                              float* __restrict__ color, float* __restrict__ depth, float* __restrict__ occ) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)4 * H * W;
    if (i >= n) return;
    const int col = (int)(i % W), y = (int)((i / W) % H), pl = (int)(i / ((size_t)W * H));
    int g = 0;
    while (g + 1 < G && col >= ed.e[g + 1]) g++;
    const float v = blocks[(size_t)g * stride + ((size_t)pl * H + y) * wmax + (col - ed.e[g])];
    const size_t pix = (size_t)y * W + col;
    if (pl < 2) color[(size_t)pl * H * W + pix] = v;
    else if (pl == 2) depth[pix] = v;
    else occ[pix] = v;
}
extern "C" int lidargs_wedge_unpack_columns(int G, int height, int width, int wmax, size_t block_stride, const int* edges_host, const float* blocks,
                                            float* color, float* depth, float* occ, void* stream) {
    if (G < 1 || G > 64 || height <= 0 || width <= 0 || wmax <= 0 || !edges_host || !blocks || !color || !depth || !occ || block_stride < (size_t)4 * height * wmax)
        return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_unpack_columns: bad argument");
    if (edges_host[0] != 0 || edges_host[G] != width) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_unpack_columns: edges must run from 0 to width");
    for (int g = 0; g < G; g++)
        if (edges_host[g + 1] <= edges_host[g] || edges_host[g + 1] - edges_host[g] > wmax) return api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "wedge_unpack_columns: bad edges");
    WedgeEdges ed;
    for (int g = 0; g <= G; g++) ed.e[g] = edges_host[g];
    const size_t n = (size_t)4 * height * width;
    hipLaunchKernelGGL(k_wedge_unpack_columns, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, height, width, wmax, block_stride, ed, blocks, color,
                       depth, occ);
    return api_check_launch((hipStream_t)stream, 0, "wedge unpack columns");
}

}  // namespace lg
