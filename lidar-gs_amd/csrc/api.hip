// api.hip -- extern "C" entry points of include/lidargs_rasterizer.h and the host-side
// stage sequence (the counterpart of CudaRasterizer::Rasterizer::{forward,backward,...},
// R3/cr/rasterizer_impl.cu:202-549): forward_impl / backward_impl and every frame that goes
// through them, the sharded path's (range shells, column wedges) included.  What the sharded
// path launches around a rank's frame -- selection, gradient rows, image folds -- is shard.hip.
//
// Differences from the reference's host sequence, all behind the same interface:
//   - everything is enqueued on the caller's stream; there is no device-wide synchronise
//     (the reference calls cudaDeviceSynchronize after most kernels, R3/cr/forward.cu:682,:753,
//     R3/cr/rasterizer_impl.cu:311, R3/cr/backward.cu:843,:870,:932);
//   - the single host wait is the 16-byte read-back of the instance count needed to size the
//     binning buffer (the reference's blocking cudaMemcpy, R3/cr/rasterizer_impl.cu:292);
//   - errors are returned as negative codes instead of printf-and-continue.
#include "lidargs_common.h"
#include "../../include/lidargs_rasterizer.h"
#include "../../include_pose/lidargs_pose.h"

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <limits>
#include <algorithm>
#include <atomic>
#include <mutex>

namespace {
using lg::SegPlan;

thread_local char g_err[512] = "";
// diagnostics of the last forward ON THIS THREAD (lidargs_last_counters); never read by the compute path
thread_local long long g_counters[10] = {0, 0, 0, 0, 0, 0, 0, 0, -1, -1};
// The device-side counters ([1], [3], [6], [8], [9]) are counted by small launches queued at the END OF THE FORWARD ITSELF, while the
// caller's buffers are by definition alive, into a page this library owns, and only when asked for (lidargs_counters_enable): nothing
// is remembered about the caller's memory, nothing is allocated per query (round-5 verdict item 9 / advisor finding).
thread_local int g_counters_on = 0;
struct CounterPage {
    unsigned long long* dev = nullptr; unsigned long long* host = nullptr; hipEvent_t done = nullptr; int device = -1; bool pending = false;
    bool ready() {
        int d = -1;
        if (hipGetDevice(&d) != hipSuccess) return false;
        if (dev && d == device) return true;
        if (dev) { (void)hipFree(dev); dev = nullptr; }
        if (done) { (void)hipEventDestroy(done); done = nullptr; }
        if (!host && hipHostMalloc((void**)&host, 8 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) { host = nullptr; return false; }
        if (hipMalloc((void**)&dev, 8 * sizeof(unsigned long long)) != hipSuccess) { dev = nullptr; return false; }
        if (hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) { done = nullptr; return false; }
        device = d; pending = false;
        return true;
    }
};
thread_local CounterPage t_cnt;

__global__ void __launch_bounds__(64) k_cnt_diag(const unsigned long long* __restrict__ slots, unsigned long long* __restrict__ out) {
    unsigned long long v = 0, r = 0;                                   // the preprocess' LG_INST_SLOTS pairs (visible, reference tiles_touched)
    for (int i = threadIdx.x; i < LG_INST_SLOTS; i += 64) { v += slots[2 * i]; r += slots[2 * i + 1]; }
    for (int o = 32; o > 0; o >>= 1) { v += __shfl_xor(v, o); r += __shfl_xor(r, o); }
    if (threadIdx.x == 0) { out[0] = v; out[1] = r; }
}
__global__ void __launch_bounds__(256) k_cnt_bytes(const uint8_t* __restrict__ p, size_t n, size_t stride, unsigned long long* __restrict__ out) {
    const uint8_t* row = p + (size_t)blockIdx.y * stride;
    uint32_t c = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) c += row[i] != 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}
}  // namespace

// queued behind a forward's last launch (see above); `view` = the selection a backward on these buffers will make, or NULL
void lg::note_forward(size_t P, size_t R, const FrameLayout& L, const uint32_t* totals, const uint8_t* flags, const uint8_t* touched,
                      const RenderBwdArgs* view, hipStream_t s) {
    g_counters[0] = (long long)P; g_counters[2] = (long long)R; g_counters[4] = L.TH; g_counters[5] = L.grid.num_tiles(); g_counters[7] = L.S;
    g_counters[1] = g_counters[3] = g_counters[8] = g_counters[9] = -1;
    g_counters[6] = flags ? -1 : 0;
    t_cnt.pending = false;
    if (!g_counters_on || !t_cnt.ready()) return;
    unsigned long long* d = t_cnt.dev;
    if (hipMemsetAsync(d, 0, 8 * sizeof *d, s) != hipSuccess) return;
    hipLaunchKernelGGL(k_cnt_diag, dim3(1), dim3(64), 0, s, reinterpret_cast<const unsigned long long*>(totals + LG_TOTALS_DIAG_WORD), d);
    if (flags && R) hipLaunchKernelGGL(k_cnt_bytes, dim3(512, L.grid.waves_per_tile), dim3(256), 0, s, flags, R, L.Rp, d + 2);
    if (touched && P) hipLaunchKernelGGL(k_cnt_bytes, dim3(512, 1), dim3(256), 0, s, touched, P, (size_t)0, d + 3);
    if (view) lg::launch_count_backward_entries(*view, d + 4, s);
    t_cnt.host[5] = (flags && R ? 1u : 0u) | (touched && P ? 2u : 0u) | (view ? 4u : 0u);     // which of the counts exist (host-side word of the same page)
    if (hipMemcpyAsync(t_cnt.host, d, 5 * sizeof *d, hipMemcpyDeviceToHost, s) != hipSuccess) return;
    if (hipEventRecord(t_cnt.done, s) != hipSuccess) return;
    t_cnt.pending = true;
}

namespace {
int fail(int code, const char* fmt, const char* detail = "") {
    snprintf(g_err, sizeof g_err, fmt, detail);
    return code;
}

#define LG_HIP(call)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return fail(LIDARGS_ERR_HIP, #call ": %s", hipGetErrorString(e_)); \
    } while (0)

int check_launch(hipStream_t s, int debug, const char* what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && debug) e = hipStreamSynchronize(s);       // CHECK_CUDA(.., debug), R3/cr/auxiliary.h:202-209
    if (e != hipSuccess) {
        snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
        return LIDARGS_ERR_HIP;
    }
    return 0;
}
#define LG_STAGE_CHECK(what)                                  \
    do {                                                      \
        int rc_ = check_launch(stream, debug, what);          \
        if (rc_) return rc_;                                  \
    } while (0)

// Tile height from the instance totals the preprocess accumulated for heights 4 / 8 / 16 / 32.  The blend costs the same for every
// height (per-lane row test + contribution flags), the binning costs ~18 ns per 1000 instances, and a taller tile makes pass 1
// visit entries that do not reach a patch's rows.  Measured: street scenes (instances shrink 1.27x / 1.46x at 8 / 16 rows) are
// fastest at 4 rows, an 8 M-Gaussian shell scene with tall footprints (1.74x / 2.77x) at 16 (4.5 -> 3.0 ms) and, its instances
// shrinking another 1.5x, at 32 (2.52 -> 2.33 ms: binning 0.53 -> 0.34 ms against 0.05 ms more in pass 1).
int choose_tile_rows(const unsigned long long (&inst)[4], int height) {
    if (const int f = lg::switches().tile_rows) return f;
    const double r4 = (double)inst[0];
    if (inst[2] > 0 && r4 / (double)inst[2] >= 2.2) {
        if (height >= 64 && inst[3] > 0 && (double)inst[2] / (double)inst[3] >= 1.4) return 32;
        return 16;
    }
    if (inst[1] > 0 && r4 / (double)inst[1] >= 1.6) return 8;
    // big frames: binning costs ~16 ns per 1000 instances (emit + two sort passes + ranges), so a smaller ratio already pays when
    // it removes >= 12 M instances (8 M street Gaussians @ 128x4096: ratio 1.56, 47.5 -> 30.4 M instances, 2.62 -> 2.41 ms)
    if (inst[1] > 0 && r4 / (double)inst[1] >= 1.4 && inst[0] - inst[1] >= 12000000ull) return 8;
    return 4;
}

// What the backward (and a shell's phase 2) must know about the forward that made its buffers travels in the one value the
// interface hands from one to the other, the `num_rendered` int (R3/rasterize_points.cu:123 -> :218; opaque to every caller):
//     num_rendered = Rp | code,   Rp = instance count rounded up to a multiple of 4,  tile height = 4 << code  (4, 8, 16, 32)
// Rp sizes and carves the binning buffer on both sides (the list itself has `ranges`), so nothing is looked up by buffer
// address and cloned / offloaded / checkpointed saved buffers work (the backward rebuilds its view from (P, R, W*H)).
// Which Gaussians have a gradient at all is a byte map IN the geometry buffer (GeomView::touched): every backward clears exactly their lines first.
inline int encode_rendered(size_t R, int TH) { return (int)(((R + 3) & ~(size_t)3) | (size_t)(TH == 8 ? 1 : (TH == 16 ? 2 : (TH == 32 ? 3 : 0)))); }

// One pinned 4-KB landing buffer and one event per host thread and device: the host waits for the copy alone, not for what
// was queued behind it.
struct HostRead {
    static constexpr int WORDS = 1024;
    uint32_t* words = nullptr; hipEvent_t copied = nullptr; int device = -1;
    bool ready() {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) return false;
        if (words && dev == device) return true;
        if (copied) { (void)hipEventDestroy(copied); copied = nullptr; }
        if (!words && hipHostMalloc((void**)&words, WORDS * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) { words = nullptr; return false; }
        if (hipEventCreateWithFlags(&copied, hipEventDisableTiming) != hipSuccess) { copied = nullptr; return false; }
        device = dev;
        return true;
    }
};
thread_local HostRead t_host_read;

// How a frame's tile lists are cut up: target entries per segment, segment slots per list, and the depth (in segments) of the
// gated pass-1 rounds, e.g. rounds {3, 9} walks segments [0,3), then [3,9) of the patches still open, then the rest of those
// still open after that.  A pure function of (R, waves per tile, variant) and the environment, so the backward and the shell's
// phase 2 find the split the forward used.
//   Few nominal segments (R * waves_per_tile / 128 < 150 k: the 2 M-Gaussian 64x2650 frames, range shells of them) leave the
//   blend latency-bound at ~2 waves per SIMD (SQ_WAVE_CYCLES), so the lists are cut finer: 64-entry segments, 45 slots, a first
//   round of 5 segments (cfg3 0.99 -> 0.93 ms).  Frames with plenty of segments (8 M Gaussians at 128x4096) lose 10 % that way
//   and keep 128 / 33 / 3.  The surfel blend does twice the arithmetic per entry and sits in between: 96 / 45 / 6.
SegPlan plan_segments(size_t R, int waves_per_tile, int surfel, size_t patches = 0) {
    const lg::Switches& env = lg::switches();
    SegPlan p;
    const bool fine = (unsigned long long)R * (unsigned)waves_per_tile / 128ull < 150000ull;
    p.seg_len = fine ? 64 : LG_SEG_LEN_DEFAULT;   // (the surfel variant took 96 until its walks got a fifth cheaper: round 4's end, 64 / 8 segments beat 96 / 6 by 1.5 %)
    p.max_segments = fine ? (surfel ? 21 : 45) : 33;        // odd: keeps the segment index decorrelated from the XCD a workgroup lands on (render.hip)
    // (surfel, round 6: with the footprint pruning its lists are 2.2 x shorter -- 21 slots and a first round of 6 segments beat 45 / 8 by 2.3 % of
    //  the cfg5 frame, 3.1 % at opacity x 0.1, 2.2 % at x 0.3; grid of {17..37} x {5, 6, 7}: tools/tune_plan_cfg5.sh, profiles/r06_tune_plan_cfg5.txt)
    // gated pass-1 rounds.  Fine plan: one round (5 segments; the surfel variant 6 of its 64-entry segments -- 8 before its lists were pruned: against 6, 10, 12 and
    // (5, 12) on cfg5, and against 6 of 96 entries; more rounds only add launch tails there).  Big frames (128-entry segments): the first segment alone, then segments [1, 4) of the patches still
    // open, then the rest -- 8 M Gaussians @ 128x4096: shell scene 2.33 -> 2.17 ms, street scene 2.62 -> 2.50 ms against {3}.
    if (fine) { p.n_rounds = 1; p.rounds[0] = surfel ? 6 : 5; }
    else { p.n_rounds = 2; p.rounds[0] = 1; p.rounds[1] = 4; }
    // Round 1 as the complete walk of the list heads (k_render_pass2_grouped<true>) instead of a T-only walk that pass 2 repeats: on
    // the big frames, whose first round is the first 128-entry segment alone (8 M Gaussians @ 128x4096: blends 0.233 -> 0.205 ms).  On
    // the 64x2650 frames a workgroup per patch walking 5 segments in a row is 2.6 waves per SIMD of serial work: 2 M Gaussians lose
    // 0.09 ms, 0.5 M are even; heads of 1 or 2 segments there lose 0.03-0.04 ms to the extra launches (r02 measurements).
    p.head = (fine || surfel) ? 0 : 1;
    if (env.head >= 0 && !surfel) p.head = env.head ? 1 : 0;
    // Small frames (<= 1 M instances: per-rank sub-frames of a sharded scene, small scenes) run the fine plan's forward blend as ONE
    // launch, a workgroup of 8 waves per patch walking the list in rounds of 8 segments (render.hip k_render_fused): the records are
    // gathered once instead of 2-3 times, there are no workgroups that only read a range and retire, and five launches become one.
    // Measured (r03): 0.17 M instances 0.095 -> 0.057 ms, 0.7 M 0.137 -> 0.114 ms; at 1.3 M (0.165 -> 0.196 ms) and 5.7 M
    // (0.195 -> 0.252 ms) the few long unsaturated lists, walked round after round by one workgroup, are a tail the multi-launch
    // form does not have.  The two forms produce bit-identical images.  LIDARGS_FUSED = 0 / 1 forces one of them.
    // ... and short lists (<= 600 instances per patch the launch covers on average): a column wedge of a sharded frame has few
    // instances but the single-GPU frame's long lists, and its 300-odd patches leave nothing to hide the long ones' rounds behind
    // (8 wedges of the 2 M frame: kernel stages 0.41 -> 0.47 ms per rank with the fused form, r03 replay)
    p.fused = (fine && !surfel && R <= (size_t)1000000 && (patches == 0 || R <= 600 * patches)) ? 1 : 0;
    if (env.fused >= 0 && !surfel) p.fused = env.fused ? 1 : 0;
    if (env.seg_len) p.seg_len = env.seg_len;
    if (env.max_segments) p.max_segments = env.max_segments;
    if (env.n_rounds >= 0) { p.n_rounds = env.n_rounds; for (int k = 0; k < env.n_rounds; k++) p.rounds[k] = env.rounds[k]; }
    return p;
}

// Pass 1 in rounds of growing depth: the first segments of every list, then -- only for the patches some pixel of which is
// still unsaturated -- the next ones, and so on.  In a street scene most patches saturate within a few hundred entries,
// and pass 1 (which restarts from T = 1 in every segment) would otherwise walk every entry behind that point for nothing.
// Leaves `ra` covering all segments with the gate armed, which is what pass 2 and the combine expect.
// `head` (out, nullable): when the caller goes on to pass 2 and the walk starts from T = 1, the first round is not a T-only walk but
// the head of every list walked once, completely (render.hip k_render_pass2_grouped<true>); *head = its segments, which pass 2 then
// skips.  0 = no head (plans without one, transmittance-only passes, walks that start from a T_in plane).
void run_pass1_rounds(lg::RenderFwdArgs& ra, const SegPlan& plan, uint8_t* alive, hipStream_t stream, int* head = nullptr) {
    const int S = ra.S;
    const int* r = plan.rounds;
    const int n = plan.n_rounds;
    ra.alive = nullptr; ra.front = 0;
    int lo = 0;
    if (head) *head = 0;
    for (int i = 0; i < n && r[i] < S; i++) {
        ra.seg_lo = lo; ra.seg_hi = r[i];
        if (i == 0 && head && plan.head && !ra.T_in && !ra.transmittance_only && ra.flags) {
            lg::launch_render_head(ra, r[0], stream);
            *head = r[0];
        } else {
            lg::launch_render_pass1(ra, stream);   // gated on the limits the previous rounds left (none in the first)
        }
        ra.alive = alive; ra.front = r[i];
        lg::launch_render_alive(ra, stream);
        lo = r[i];
    }
    ra.seg_lo = lo; ra.seg_hi = S;
    lg::launch_render_pass1(ra, stream);
    ra.seg_lo = 0; ra.seg_hi = S;
}

int ceil_log2(uint32_t n) {
    int b = 0;
    while ((1u << b) < n && b < 31) b++;
    return b;
}

// The same read in two halves: the copy is queued at `begin`, more work is queued behind it, and `end` waits for the copy only.
int read_words_begin(const uint32_t* dev, int n, hipStream_t s) {
    if (n > HostRead::WORDS || !t_host_read.ready()) return (int)hipErrorOutOfMemory;
    hipError_t e = hipMemcpyAsync(t_host_read.words, dev, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(t_host_read.copied, s);
    return (int)e;
}
int read_words_end(int n, uint32_t* out) {
    const hipError_t e = hipEventSynchronize(t_host_read.copied);
    if (e == hipSuccess) memcpy(out, t_host_read.words, (size_t)n * sizeof(uint32_t));
    return (int)e;
}

// ---- per-stage event timing -------------------------------------------------------------------
// While enabled, every forward/backward call records one HIP event per stage boundary on the op's
// own stream into a fresh slot; nothing is waited for until lidargs_profile_read()/summary().
struct Profiler {
    static constexpr int MAX_CALLS = 256;
    struct Call { int n = 0; const char* names[LIDARGS_MAX_STAGES]; hipEvent_t ev[LIDARGS_MAX_STAGES + 1]; bool created = false; };
    bool enabled = false;
    int every = 1;           // record every `every`-th call of a kind: an event costs ~4.5 us of device time, a dozen per call 6 % of a frame
    int seen[2] = {0, 0};    // calls of each kind (0 forward-like, 1 backward) since enable
    int ncalls = 0;          // calls recorded since enable
    Call* calls = nullptr;
    Call* cur = nullptr;
};
Profiler g_prof;   // process-wide: autograd runs backward on its own thread
}  // namespace

// helpers shared with the other entry-point files
namespace lg {
int api_fail(int code, const char* msg) { return fail(code, "%s", msg); }
int api_check_launch(hipStream_t s, int debug, const char* what) { return check_launch(s, debug, what); }
// Has ANY forward of this process made deterministic buffers?  Until one has, no buffer a backward of this process can be handed is
// deterministic, and backward_impl neither queues the second walk nor hands its kernels the mode word: the default mode then runs
// exactly the launches it ran before the mode existed.  Not per-forward state (it is never cleared, names no buffer and decides no
// result: with it set, the buffer's word decides as always) -- only the licence to skip a launch that would retire at once.
std::atomic<bool> g_deterministic_seen{false};
// The forwards the mode does not cover yet refuse it, before any device work: running their float-atomic backward under a switch that
// promises the opposite would be worse than an error.
int refuse_deterministic(const char* entry) {
    if (!deterministic_requested()) return 0;
    return fail(LIDARGS_ERR_INVALID_ARGUMENT, "%s: LIDARGS_DETERMINISTIC=1 is not supported by this entry point (only lidargs_forward / lidargs_backward are); unset it for this call", entry);
}
// LIDARGS_DEPTH=median / strongest / second, the same way: set by the first forward whose depth is one Gaussian's range (each value makes
// "median buffers": LG_MODE_MEDIAN and the id plane), never cleared.  Until then a backward launches exactly what it launched before
// the modes existed; from then on the first blend walk asks the buffer's mode word and k_median_backward is queued (it retires on one
// load on a default buffer).  The buffer's word decides every result, not this flag.
std::atomic<bool> g_median_seen{false};
int refuse_depth_mode(const char* entry) {
    if (!picked(depth_mode())) return 0;
    return fail(LIDARGS_ERR_INVALID_ARGUMENT, "%s: a non-default LIDARGS_DEPTH (" LG_PICKED_DEPTH_NAMES ") is not supported by this entry point (only lidargs_forward / lidargs_backward are); unset it for this call", entry);
}
int api_read_words_zero_behind(const uint32_t* dev, int n, uint32_t* out, void* zero, size_t zero_bytes, hipStream_t s) {
    hipError_t e = (hipError_t)read_words_begin(dev, n, s);
    if (e == hipSuccess && zero && zero_bytes) e = hipMemsetAsync(zero, 0, zero_bytes, s);
    return e == hipSuccess ? read_words_end(n, out) : (int)e;
}
bool prune_footprints() { return !switches().no_prune; }
int tile_rows() { return switches().tile_rows ? switches().tile_rows : 4; }      // what non-adaptive callers (surfel variant) use

FrameLayout frame_layout(int num_rendered, int W, int H, int col_lo, int col_hi, FrameVariant variant) {
    const bool surfel = variant == FRAME_SURFEL, shell = variant == FRAME_SHELL;
    FrameLayout L;
    L.TH = 4 << (num_rendered & 3);                       // (encode_rendered)
    L.Rp = (size_t)(num_rendered & ~3);
    L.grid = make_grid(W, H, L.TH);
    if (col_lo >= 0) { L.grid.x_lo = col_lo / LG_TILE_W; L.grid.x_n = (col_hi + LG_TILE_W - 1) / LG_TILE_W - L.grid.x_lo; }   // the blends cover the wedge's own tile columns only
    L.patches = (size_t)L.grid.num_tiles() * L.grid.waves_per_tile;
    L.plan = surfel ? plan_segments(L.Rp, L.grid.waves_per_tile, 1) : plan_segments(L.Rp, L.grid.waves_per_tile, 0, (size_t)L.grid.window_patches());
    L.S = choose_segments(L.Rp, L.plan.max_segments);
    L.fused = L.plan.fused && !shell;                     // the plain frame (a range shell's two phases keep the launches; surfel plans are never fused)
    L.gated = L.fused || (L.plan.n_rounds > 0 && L.plan.rounds[0] < L.S);
    L.flags = L.fused || L.S > 1 || shell || surfel;      // a shell's backward always reads the flags; the surfel forward always runs pass 1
    // The backward blend walks the work list k_render_combine filled (lidargs_common.h WorkList) on every plain or column-wedge frame that
    // runs the segmented launches (a shell's backward keeps the slot grid).  LIDARGS_WORK_LISTS=0: the slot grid again (A/B, tests).
    L.work_list = switches().work_lists && !surfel && !shell && work_lists_fit(L.patches, L.S) && !L.fused && L.S > 1;
    L.buf = surfel ? SURFEL_BUFFERS : GAUSS_BUFFERS;
    return L;
}
void prof_begin(hipStream_t s, int kind) {
    Profiler& p = g_prof;
    p.cur = nullptr;
    if (!p.enabled) return;
    if (p.seen[kind]++ % p.every != 0) return;
    if (!p.calls) p.calls = new Profiler::Call[Profiler::MAX_CALLS];
    p.cur = &p.calls[p.ncalls % Profiler::MAX_CALLS];
    p.ncalls++;
    if (!p.cur->created) { for (auto& e : p.cur->ev) (void)hipEventCreate(&e); p.cur->created = true; }
    p.cur->n = 0;
    (void)hipEventRecord(p.cur->ev[0], s);
}
void prof_mark(const char* name, hipStream_t s) {
    Profiler::Call* c = g_prof.cur;
    if (!c || c->n >= LIDARGS_MAX_STAGES) return;
    c->names[c->n] = name;
    (void)hipEventRecord(c->ev[c->n + 1], s);
    c->n++;
}

// The binning sequence of both rasterizers' forwards (lidargs_common.h BinSpec): the preprocess has run and left the instance totals,
// key span and spans in the geometry buffer.
int bin_frame(const BinSpec& spec, const GeomView& geom, uint2* ranges, size_t P, int W, int H, int col_lo, int col_hi, bool compact,
              char* (*binning_alloc)(void*, size_t), void* binning_user, int debug, hipStream_t stream, BinnedFrame* out) {
    const bool enqueue_only = spec.capacity > 0, surfel = spec.variant == FRAME_SURFEL;
    // 1. range sort of the Gaussians on the low 31 key bits (8 + 8 + 8 + 7 by default; LIDARGS_RANGE_SORT_BITS=11 gives 11 + 10 + 10, slower
    //    at 2 M keys): ranges are positive floats (bit 31 clear), and a culled Gaussian's key 0xFFFFFFFF still sorts behind every
    //    valid one (valid keys are < bits(lidar_far) < 0x7FFFFFFF)
    //    Everything the host decides on -- the instance totals per tile height -- is known once the preprocess has run: their copy
    //    (2 KB into pinned memory) is queued here, the sort behind it, and the host waits for the copy while the sort runs.
    if (!enqueue_only) LG_HIP((hipError_t)read_words_begin(geom.totals, LG_TOTALS_READ_WORDS, stream));
    RadixTail span_tail;                                               // the sort's last pass leaves the spans in range order as well
    span_tail.src = geom.spans; span_tail.dst = geom.span_sorted; span_tail.mode = compact ? 1 : 2;
    const uint32_t* ids_sorted = geom.id_a;
    int first_side = 1;                                                // where the first pass left the pairs (0: a side, 1: b side)
    // The sort runs on key - kmin (the preprocess left ~kmin and kmax in the totals' slots): a frame's ranges span far fewer than 31 key
    // bits -- 2 m .. 80 m is 26 -- and every 8-9 bits less is a pass (three launches) less.  kmin is rounded down to a multiple of 256,
    // so the first pass (the key's own low byte) needs no host knowledge and is queued right behind the totals' copy; the host then
    // reads the span and queues as many more passes as it has bits.
    // Round 5: frames of up to 4 M Gaussians sort in ONE bucket pass + one launch that finishes every bucket in LDS (binning.hip
    // launch_range_sort_buckets), with the frame's range span folded on the device: queued whole behind the totals' copy.
    const bool buckets = range_sort_buckets_ok(P);
    if (buckets) {
        launch_range_sort_buckets(geom.key_a, geom.key_b, geom.id_a, geom.id_b, P, geom.scratch, geom.totals + LG_TOTALS_KEYSPAN_WORD, span_tail, stream);
        LG_STAGE_CHECK("range sort");
    } else if (enqueue_only) {                                         // no host read: all 31 bits of the raw key
        const int side = launch_radix_sort_pairs(geom.key_a, geom.key_b, geom.id_a, geom.id_b, P, 31, geom.scratch, stream,
                                                 switches().range_sort_bits, nullptr, SORT_MAX_RADIX_BITS, true, span_tail);   // (scratch carved for 11-bit digits; ids = positions)
        ids_sorted = side ? geom.id_b : geom.id_a;
        LG_STAGE_CHECK("range sort");
    } else {
        // (its result side is kept: one pass of the general form ends on the b side, the single-launch form of small inputs on the a side)
        first_side = launch_radix_sort_pairs(geom.key_a, geom.key_b, geom.id_a, geom.id_b, P, 8, geom.scratch, stream, 8, nullptr,
                                             SORT_MAX_RADIX_BITS, true);
        LG_STAGE_CHECK("range sort, first pass");
    }

    // 2. the one host wait (R3/cr/rasterizer_impl.cu:292), for a copy that was queued before the sort: the instance totals for tile
    //    heights 4 / 8 / 16 / 32 -> tile height, R; then the instance offsets in range order for that height.  The device is still
    //    sorting while the host decides and queues what follows (the packed gradient lines are zeroed by the preprocess itself, so
    //    there is no fill to queue behind the copy any more, and no guess of the tile height).
    uint32_t totals_h[LG_TOTALS_READ_WORDS];                           // the slots of 64-bit instance totals the preprocess filled
    if (!enqueue_only) {
        LG_HIP((hipError_t)read_words_end(LG_TOTALS_READ_WORDS, totals_h));
        if (!buckets) {   // the rest of the range sort: bits [8, bits of (kmax - kmin + 1)) in passes of at most 9 bits; at least one pass, for the tail
            uint32_t kinv = 0u, kmax = 0u;
            for (int slot = 0; slot < LG_INST_SLOTS; slot++) {
                kinv = std::max(kinv, totals_h[LG_TOTALS_KEYSPAN_WORD + 2 * slot]); kmax = std::max(kmax, totals_h[LG_TOTALS_KEYSPAN_WORD + 2 * slot + 1]);
            }
            const RangeSortRest rest = range_sort_rest(kinv, kmax);
            KeyBias kb = rest.bias;
            int bits = rest.end_bit;
            const bool env_full = switches().range_sort_full;              // LIDARGS_RANGE_SORT_FULL=1: always 31 bits (A/B)
            if (env_full && !surfel) { bits = 32; kb.kmin = 0u; kb.cull = 0xFFFFFFFFu; }
            uint32_t* const k_in = first_side ? geom.key_b : geom.key_a; uint32_t* const k_out = first_side ? geom.key_a : geom.key_b;
            uint32_t* const v_in = first_side ? geom.id_b : geom.id_a; uint32_t* const v_out = first_side ? geom.id_a : geom.id_b;
            const int side = launch_radix_sort_pairs(k_in, k_out, v_in, v_out, P, bits, geom.scratch, stream,
                                                     env_full && !surfel ? 8 : rest.max_bits, nullptr, SORT_MAX_RADIX_BITS, false, span_tail, 8, &kb);
            ids_sorted = side ? v_out : v_in;
            LG_STAGE_CHECK("range sort");
        }
    }
    prof_mark("range_sort", stream);
    int TH = spec.tile_rows;
    size_t R;
    uint32_t* status_dev = geom.totals + LG_TOTALS_STATUS_WORD;
    if (!enqueue_only) {
        unsigned long long inst[4] = {0, 0, 0, 0};
        for (int slot = 0; slot < LG_INST_SLOTS; slot++) {
            unsigned long long v[4];
            memcpy(v, totals_h + LG_TOTALS_SLOT_WORD + 8 * slot, sizeof v);
            inst[0] += v[0]; inst[1] += v[1]; inst[2] += v[2]; inst[3] += v[3];
        }
        if (!TH) TH = choose_tile_rows(inst, H);                       // 4, 8, 16 or 32
        // (the surfel preprocess sums the instances of its one tile height in word 0 of each slot)
        const unsigned long long R64 = (surfel || TH == 4) ? inst[0] : (TH == 8 ? inst[1] : (TH == 16 ? inst[2] : inst[3]));
        if (R64 > (unsigned long long)std::numeric_limits<int>::max() - 4ull) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "%s: instance count overflows int", spec.what);
        R = (size_t)R64;
        launch_instance_offsets(geom.span_sorted, compact, TH, geom.block_off, geom.totals, P, stream, false);   // (the host has R from the preprocess's totals; the emit adds the block sums up itself)
        LG_STAGE_CHECK("instance scan");
    } else {
        // the capacity, rounded up to the multiple of 4 `num_rendered` can carry, stands in for the count everywhere on the host: the
        // emit's cap, k_finish_totals' cap, the tile sort, the tile ranges and the buffer carving all see this ONE number (round 2
        // sorted and ranged only the unrounded capacity: need in (capacity, rounded] dropped instances with no overflow flag)
        R = ((size_t)spec.capacity + 3) & ~(size_t)3;
        launch_instance_offsets(geom.span_sorted, compact, TH, geom.block_off, geom.totals, P, stream);
        LG_STAGE_CHECK("instance scan");
        launch_finish_totals(geom.totals, reinterpret_cast<const unsigned long long*>(geom.totals + LG_TOTALS_SLOT_WORD), (uint32_t)R, status_dev, stream);
        if (spec.status_host) LG_HIP(hipMemcpyAsync(spec.status_host, status_dev, LG_STATUS_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    const uint32_t* R_dev = enqueue_only ? status_dev + 1 : nullptr;   // instances binned = min(needed, capacity), on the device
    prof_mark("scan+readback", stream);

    // everything a later call on these buffers derives (plan, carving, flag stride) comes from the returned int alone
    const int rendered = encode_rendered(R, TH);
    const FrameLayout& L = out->L = frame_layout(rendered, W, H, col_lo, col_hi, spec.variant);
    out->R = R;
    char* bin_p = binning_alloc(binning_user, L.bin_carve(nullptr, nullptr));
    if (!bin_p) return fail(LIDARGS_ERR_ALLOC, "%s: binning allocator returned NULL", spec.what);
    BinView& bin = out->bin;
    L.bin_carve(bin_p, &bin);

    // 3. emit instances in range order, bin them by tile (stable); 16-bit tile keys whenever the tile ids fit (LIDARGS_TILE_KEY32=1: A/B)
    const int tiles = L.grid.num_tiles();
    const bool key16 = tiles <= 65536 && (surfel || !switches().tile_key32);
    if (R) {
        // the sorted lists are wanted on the a side (the backward finds them there whatever the pass count was): a sort that will end on
        // the other side -- an odd number of passes: images of at most 256 list tiles -- gets its input there, instead of two copies behind it
        const int bits = ceil_log2((uint32_t)tiles);
        const bool flip = radix_sort_result_side(R, bits) != 0;
        uint32_t* const k_in = flip ? bin.tile_b : bin.tile_a; uint32_t* const k_out = flip ? bin.tile_a : bin.tile_b;
        uint32_t* const v_in = flip ? bin.val_b : bin.val_a; uint32_t* const v_out = flip ? bin.val_a : bin.val_b;
        launch_emit_instances(ids_sorted, geom.block_off, geom.span_sorted, compact, P, L.grid, k_in, v_in, stream,
                              enqueue_only ? (uint32_t)L.Rp : 0xFFFFFFFFu, key16, ranges, !enqueue_only);
        LG_STAGE_CHECK("emit");
        prof_mark("emit", stream);
        const int side = key16 ? launch_radix_sort_pairs16(reinterpret_cast<uint16_t*>(k_in), reinterpret_cast<uint16_t*>(k_out), v_in, v_out, R,
                                                           bits, bin.scratch, stream, R_dev)
                               : launch_radix_sort_pairs(k_in, k_out, v_in, v_out, R, bits, bin.scratch, stream, 0, R_dev);
        const int bside = side ^ (flip ? 1 : 0);                       // 1: the result is NOT on the a side after all (never, by radix_sort_result_side)
        if (bside) {   // keep the backward's view independent of the pass count: result always in (tile_a, val_a)
            LG_HIP(hipMemcpyAsync(bin.tile_a, bin.tile_b, R * (key16 ? sizeof(uint16_t) : sizeof(uint32_t)), hipMemcpyDeviceToDevice, stream));
            LG_HIP(hipMemcpyAsync(bin.val_a, bin.val_b, R * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        }
        LG_STAGE_CHECK("tile bin");
        prof_mark("tile_bin", stream);
    }
    // (the launch also clears the counters of the backward's work list, where there is one: nothing before the blends touches them)
    launch_tile_ranges(bin.tile_a, R, ranges, tiles, stream, R_dev, key16, bin.work, bin.work ? LG_WORK_REGIONS * LG_WORK_CNT_STRIDE : 0, R != 0);
    LG_STAGE_CHECK("tile ranges");
    prof_mark("ranges", stream);
    return rendered;
}
}  // namespace lg

namespace {

// ---- a frame's arguments, stated once ---------------------------------------------------------------------------------------------
// Every entry point fills these values BY FIELD NAME from its C parameter list and hands them on whole, so nothing in the host sequence hangs on an
// argument's position (two swapped float* compile cleanly and show up as a wrong gradient).  What a frame does not have stays NULL / 0.
struct FrameAllocs { lidargs_alloc_fn geometry = nullptr, binning = nullptr, image = nullptr; void* geometry_user = nullptr; void* binning_user = nullptr; void* image_user = nullptr; };
// The scene and the sensor, for the forward and the backward alike: a backward, and the per-Gaussian chain's test hooks, leave unset what they do not read.
struct SceneArgs {
    int P = 0, width = 0, height = 0; float scale_modifier = 1.f, near_f = 0.f, far_f = 0.f;
    const float* background = nullptr; const float* means3D = nullptr; const float* colors_precomp = nullptr; const float* opacities = nullptr;
    const float* scales = nullptr; const float* rotations = nullptr; const float* cov3D_precomp = nullptr; const float* viewmatrix = nullptr; const float* beams = nullptr;
};
struct FrameOutputs { float* out_color = nullptr; float* out_depth = nullptr; float* out_occ = nullptr; int* radii = nullptr; int* radii_xy = nullptr; };
struct SavedFrame {   // what a forward left for its backward
    int R = 0; const int* radii = nullptr; char* geom_buffer = nullptr; char* binning_buffer = nullptr; char* image_buffer = nullptr; };
// A backward's twelve gradient rows.  dL_dconic, dL_ddepths, dL_dsphere_means3D, dL_dbasis_u1/u2 are the reference's scratch gradients: optional (NULL = not materialised).
struct GradRows {
    float* dL_dmean2D = nullptr; float* dL_dconic = nullptr; float* dL_dopacity = nullptr; float* dL_dcolor = nullptr; float* dL_ddepths = nullptr; float* dL_dmean3D = nullptr;
    float* dL_dsphere_means3D = nullptr; float* dL_dbasis_u1 = nullptr; float* dL_dbasis_u2 = nullptr; float* dL_dcov3D = nullptr; float* dL_dscale = nullptr; float* dL_drot = nullptr;
    bool required(const float* cov3D_precomp) const { return dL_dmean2D && dL_dopacity && dL_dcolor && dL_dmean3D && dL_dscale && dL_drot && (!cov3D_precomp || dL_dcov3D); }
    lg::ZeroRows zero_rows() const {   // what a backward's first launch zeroes, with the rows' widths
        lg::ZeroRows zr; zr.add(dL_dmean2D, 4); zr.add(dL_dconic, 4); zr.add(dL_dopacity, 1); zr.add(dL_dcolor, 2); zr.add(dL_ddepths, 1); zr.add(dL_dmean3D, 3);
        zr.add(dL_dsphere_means3D, 3); zr.add(dL_dbasis_u1, 3); zr.add(dL_dbasis_u2, 3); zr.add(dL_dcov3D, 6); zr.add(dL_dscale, 3); zr.add(dL_drot, 4);
        return zr;
    }
};
struct FrameGrads {   // in per pixel, out per Gaussian
    const float* dL_dpix = nullptr; const float* dL_dout_depth = nullptr; const float* dL_dout_occ = nullptr; GradRows rows; };

// The per-Gaussian chain's arguments from (scene, gradient rows, packed sums and touched lists); radii, det_mode, acc64, view_partials: each caller's own.
lg::GaussBwdArgs gauss_bwd_args(const SceneArgs& sc, const GradRows& g, const float* gacc, const uint8_t* tlist, const uint16_t* tcount) {
    lg::GaussBwdArgs gb;
    gb.P = sc.P; gb.scale_modifier = sc.scale_modifier; gb.view = sc.viewmatrix; gb.gacc = gacc; gb.tlist = tlist; gb.tcount = tcount;
    gb.means3D = sc.means3D; gb.scales = sc.scales; gb.rotations = sc.rotations; gb.cov3D_precomp = sc.cov3D_precomp; gb.dL_dmean2D = g.dL_dmean2D; gb.dL_dconic = g.dL_dconic; gb.dL_dopacity = g.dL_dopacity; gb.dL_dcolor = g.dL_dcolor; gb.dL_ddepths = g.dL_ddepths;
    gb.dL_dbasis_u1 = g.dL_dbasis_u1; gb.dL_dbasis_u2 = g.dL_dbasis_u2; gb.dL_dsphere = g.dL_dsphere_means3D; gb.dL_dmean3D = g.dL_dmean3D;
    gb.dL_dcov3D = g.dL_dcov3D; gb.dL_dscale = g.dL_dscale; gb.dL_drot = g.dL_drot;
    return gb;
}
// What a blend of a frame's lists takes from (layout, the three buffer views, background, outputs), covering every segment.  What the
// plain forward and a shell's phase 2 differ in -- run_pass1, flags, alive, T_end_out, fill -- and the T planes are each site's own.
lg::RenderFwdArgs render_fwd_args(const lg::FrameLayout& L, const lg::GeomView& geom, const lg::BinView& bin, const lg::ImgView& img,
                                  const float* background, const FrameOutputs& out) {
    lg::RenderFwdArgs ra;
    ra.grid = L.grid; ra.ranges = img.ranges; ra.point_list = bin.val_a; ra.rec = geom.rec; ra.rowspan = geom.rowspan;
    ra.coltab = img.coltab; ra.rowtab = img.rowtab; ra.bg = background; ra.final_T = img.final_T;
    ra.out_color = out.out_color; ra.out_depth = out.out_depth; ra.out_occ = out.out_occ;
    ra.seg = bin.seg; ra.S = L.S; ra.seg_len = L.plan.seg_len; ra.R = L.Rp; ra.seg_lo = 0; ra.seg_hi = L.S; ra.front = 0;
    ra.touched = geom.touched;                                         // marked wherever a contribution flag is set (cleared by the preprocess)
    return ra;
}
// The selection a backward on a frame's buffers makes: which lists, which segments of them, behind which limits and flags.  The forward
// counts with it (note_forward) and backward_impl walks with it, so the two cannot differ.
lg::RenderBwdArgs backward_selection(const lg::FrameLayout& L, const lg::ImgView& img, const lg::BinView& bin) {
    lg::RenderBwdArgs v = lg::RenderBwdArgs();
    v.walk.cnt = nullptr; v.grid = L.grid; v.ranges = img.ranges; v.seg = bin.seg; v.S = L.S; v.seg_len = L.plan.seg_len; v.R = L.Rp;
    v.alive = L.gated ? bin.alive : nullptr; v.flags = L.flags ? bin.flags : nullptr;
    return v;
}

// Which kind of frame a forward entry point asks forward_impl for, and what only some kinds have: filled by field name like the rest.
struct FrameMode {
    // > 0: ENQUEUE-ONLY mode.  Nothing is read back: the binning buffer is sized for `instance_capacity` instances at the caller's
    // tile height (fixed_tile_rows: 4, 8, 16 or 32), every count the later stages need stays on the device, and the 16 status words
    // (binning.hip k_finish_totals: instances needed / binned, totals per tile height, overflow flag) are copied to `status_host`
    // (pinned, optional) by the stream.  The call can therefore be captured in a HIP graph.
    long long instance_capacity = 0;
    int fixed_tile_rows = 0;
    unsigned* status_host = nullptr;
    int col_lo = -1, col_hi = -1;        // >= 0: a column wedge, only the tile columns of pixel columns [col_lo, col_hi) are binned and rendered
    // The call comes from lidargs_forward_shell*.  Its backward (lidargs_backward_shell) walks the slot grid with the flags and limits of
    // the segmented launches, whatever T_in / T_out / transmittance_pass were -- a first or only shell passes none of them -- so the
    // mode is the entry point's, not inferred from those arguments (round-3 advisor finding: a direct ABI caller of a single shell got
    // the fused blend and a work list here, and a backward that read planes and flags the fused blend never wrote).
    bool is_shell = false;
    // A shell's own arguments (the defaults are the plain frame's): only Gaussians whose range lies in [shell_lo, shell_hi) are rendered, the
    // walk starts from the T_in plane (NULL = 1), a transmittance pass produces T_out alone.
    float shell_lo = -std::numeric_limits<float>::infinity(), shell_hi = std::numeric_limits<float>::infinity();
    const float* T_in = nullptr; int transmittance_pass = 0; float* T_out = nullptr;
    // device word, optional: the P rows are a capacity-sized selection of which only the first *n_valid exist (enqueue-only rank frames
    // of the sharded path): the preprocess culls the rest before reading them, everything behind it sees culled Gaussians.
    const uint32_t* n_valid = nullptr;
    // lidargs_forward under LIDARGS_DETERMINISTIC=1: the geometry buffer is asked for with its 64-bit accumulator lines behind everything
    // else and its mode word set (lidargs_common.h LG_TOTALS_MODE_WORD); every backward on these buffers then adds up in fixed point.
    bool deterministic = false;
    // lidargs_forward under a picked LIDARGS_DEPTH (switches.h DepthMode: anything but Expected) -- the depth is one Gaussian's range: the
    // image buffer is asked for with the median_id plane behind everything else, the mode word gets LG_MODE_MEDIAN ("median buffers",
    // whichever rule picked), and launch_render_picked overwrites out_depth behind the blend by the mode's rule (never together with
    // `deterministic`).  `return_gap` (LIDARGS_RETURN_GAP, metres) is read by Second alone, and is the forward's alone: the buffers do not carry it.
    lg::DepthMode depth = lg::DepthMode::Expected;
    float return_gap = 0.f;
};
// by lg::DepthMode: what launch_render_picked's launch is called in a stage check's error and in the profile (Expected has no such launch)
const struct { const char* check; const char* mark; } PICKED_STAGE[] = {
    {nullptr, nullptr}, {"render median", "render_median"}, {"render strongest", "render_strongest"}, {"render second", "render_second"}};
static_assert(sizeof(PICKED_STAGE) / sizeof(PICKED_STAGE[0]) == lg::DEPTH_MODE_COUNT, "one stage per lg::DepthMode");

// The preprocess' parameters of a whole frame on `grid`: no column wedge, full span records, pruning on, every row valid.  The forward,
// the visible filter and the test hook (lidargs_debug_preprocess) all start from here, so the column steps are the same values for each.
lg::PreprocessParams preprocess_params(int P, const lg::TileGrid& grid, float scale_modifier, float near_f, float far_f, float shell_lo,
                                       float shell_hi, const float* viewmatrix) {
    lg::PreprocessParams pp;
    pp.P = P; pp.W = grid.W; pp.H = grid.H; pp.TH = grid.TH; pp.tiles_x = grid.tiles_x; pp.tiles_y = grid.tiles_y;
    pp.scale_modifier = scale_modifier;
    pp.near_f = near_f; pp.far_f = far_f; pp.shell_lo = shell_lo; pp.shell_hi = shell_hi;
    pp.tile_x_lo = 0; pp.tile_x_hi = grid.tiles_x; pp.compact = 0; pp.prune = 1;
    const float pi_f = 3.14159265358979323846f;
    pp.col_step = 2 * pi_f / grid.W; pp.inv_col_step = (1.f / pp.col_step) * 1.000001f;                                  // R3/cr/forward.cu:334
    pp.tan_col_step = tanf(2 * pi_f / grid.W);                         // R3/cr/forward.cu:362
    pp.view = viewmatrix;
    pp.n_valid = nullptr;
    return pp;
}

int forward_impl(const FrameAllocs alloc, const SceneArgs sc, const FrameOutputs out, const FrameMode mode, int debug, hipStream_t stream) {
    const int P = sc.P, width = sc.width, height = sc.height;
    const long long instance_capacity = mode.instance_capacity;
    const int fixed_tile_rows = mode.fixed_tile_rows, col_lo = mode.col_lo, col_hi = mode.col_hi, transmittance_pass = mode.transmittance_pass;
    const bool is_shell = mode.is_shell, enqueue_only = instance_capacity > 0;
    if (enqueue_only && !(fixed_tile_rows == 4 || fixed_tile_rows == 8 || fixed_tile_rows == 16 || fixed_tile_rows == 32))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward (enqueue-only): tile_rows must be 4, 8, 16 or 32%s");
    if (enqueue_only && instance_capacity > (long long)std::numeric_limits<int>::max() - 4) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward (enqueue-only): capacity overflows int%s");
    if (P < 0 || width <= 0 || height <= 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward: bad sizes%s");
    if (height < 2) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward: need at least 2 beams%s");
    if (height > 65535 || width > 65535 * 16) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward: image too large%s");
    if (sc.colors_precomp == nullptr) return fail(LIDARGS_ERR_NO_COLORS, "For non-RGB, provide precomputed Gaussian colors!%s");
    if (!sc.means3D || !sc.opacities || !sc.viewmatrix || !sc.beams || !out.out_color || !out.out_depth || !out.out_occ || !out.radii)   // radii_xy: optional
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward: NULL required pointer%s");
    if (!sc.cov3D_precomp && (!sc.scales || !sc.rotations)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward: need scales+rotations or cov3D_precomp%s");
    if (!alloc.geometry || !alloc.binning || !alloc.image) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward: NULL allocator%s");
    if (P == 0) return 0;   // R3/rasterize_points.cu:87: outputs stay as the caller initialised them

    const lg::TileGrid grid4 = lg::make_grid(width, height, 4);        // the image buffer is laid out for the finest tiling
    lg::prof_begin(stream, 0);

    char* geom_p = alloc.geometry(alloc.geometry_user, lg::geom_carve(nullptr, (size_t)P, lg::GAUSS_BUFFERS, nullptr, mode.deterministic));
    if (!geom_p) return fail(LIDARGS_ERR_ALLOC, "geometry allocator returned NULL%s");
    const bool picked = lg::picked(mode.depth);
    char* img_p = alloc.image(alloc.image_user, lg::img_carve(nullptr, width, height, grid4.num_tiles(), nullptr, picked));
    if (!img_p) return fail(LIDARGS_ERR_ALLOC, "image allocator returned NULL%s");
    lg::GeomView geom; lg::geom_carve(geom_p, (size_t)P, lg::GAUSS_BUFFERS, &geom);
    lg::ImgView img; lg::img_carve(img_p, width, height, grid4.num_tiles(), &img);
    LG_HIP(hipMemsetAsync(geom.totals, 0, LG_TOTALS_WORDS * sizeof(uint32_t), stream));
    if (mode.deterministic) {
        lg::g_deterministic_seen.store(true, std::memory_order_relaxed);   // (before the buffer can reach any backward)
        LG_HIP(hipMemsetD32Async((hipDeviceptr_t)(geom.totals + LG_TOTALS_MODE_WORD), (int)lg::LG_MODE_DETERMINISTIC, 1, stream));   // (0 = the default, from the line above)
    }
    if (picked) {
        lg::g_median_seen.store(true, std::memory_order_relaxed);          // (before the buffer can reach any backward)
        LG_HIP(hipMemsetD32Async((hipDeviceptr_t)(geom.totals + LG_TOTALS_MODE_WORD), (int)lg::LG_MODE_MEDIAN, 1, stream));
    }

    lg::PreprocessParams pp = preprocess_params(P, grid4, sc.scale_modifier, sc.near_f, sc.far_f, mode.shell_lo, mode.shell_hi, sc.viewmatrix);
    pp.compact = lg::compact_spans(grid4.tiles_x, height) ? 1 : 0;
    pp.prune = lg::prune_footprints() ? 1 : 0;
    if (col_lo >= 0) {                                                   // column wedge: whole 16-pixel tile columns
        if (col_lo % LG_TILE_W || (col_hi % LG_TILE_W && col_hi != width) || col_hi <= col_lo || col_hi > width)
            return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward: a column wedge must be [multiple of 16, multiple of 16 or width)%s");
        pp.tile_x_lo = col_lo / LG_TILE_W; pp.tile_x_hi = (col_hi + LG_TILE_W - 1) / LG_TILE_W;
    }
    pp.n_valid = mode.n_valid;

    lg::launch_preprocess(pp, sc.means3D, sc.scales, sc.rotations, sc.opacities, sc.colors_precomp, sc.cov3D_precomp, sc.beams, out.radii, out.radii_xy,
                          geom, &img, false, stream);                  // also fills the pixel-ray tables of the image buffer
    LG_STAGE_CHECK("preprocess");
    lg::prof_mark("preprocess", stream);

    const lg::BinSpec spec = {is_shell ? lg::FRAME_SHELL : lg::FRAME_GAUSS, fixed_tile_rows, instance_capacity, mode.status_host, "forward"};
    lg::BinnedFrame bf;
    const int rendered = lg::bin_frame(spec, geom, img.ranges, (size_t)P, width, height, col_lo, col_hi, pp.compact != 0, alloc.binning, alloc.binning_user,
                                       debug, stream, &bf);
    if (rendered < 0) return rendered;
    const lg::FrameLayout& L = bf.L;
    const lg::BinView& bin = bf.bin;
    const size_t R = bf.R;

    lg::RenderFwdArgs ra = render_fwd_args(L, geom, bin, img, sc.background, out);
    ra.fill.cnt = nullptr; ra.T_in = mode.T_in; ra.T_pass = mode.T_out; ra.transmittance_only = transmittance_pass;
    ra.run_pass1 = (L.S > 1 || transmittance_pass || is_shell) ? 1 : 0;   // (a shell's backward always reads the flags)
    ra.flags = ra.run_pass1 ? bin.flags : nullptr; ra.alive = nullptr;
    int head = 0;                                                      // segments at the head of every list that round 1 walked completely
    // no flags (a one-segment plan: LIDARGS_MAX_SEGMENTS=1): pass 2 and the backward walk every listed entry, so every Gaussian may be added to
    if (!L.fused && !ra.run_pass1 && R) lg::launch_touch_all(geom.touched, out.radii, (size_t)P, stream);
    if (L.fused) {
        ra.flags = bin.flags; ra.alive = bin.alive;
        lg::launch_render_fused(ra, stream);
        LG_STAGE_CHECK("render fused");
        lg::prof_mark("render_fused", stream);
    } else {
    if (ra.run_pass1) {
        run_pass1_rounds(ra, L.plan, bin.alive, stream, transmittance_pass ? nullptr : &head);
        LG_STAGE_CHECK("render pass 1");
        lg::prof_mark("render_pass1", stream);
    }
    ra.seg_lo = head; ra.seg_hi = L.S;
    if (!transmittance_pass) {
        lg::launch_render_pass2(ra, stream);
        LG_STAGE_CHECK("render pass 2");
        lg::prof_mark("render_pass2", stream);
    }
    if (L.work_list) ra.fill = lg::work_list(bin);
    lg::launch_render_combine(ra, stream);
    LG_STAGE_CHECK("render combine");
    lg::prof_mark("render_combine", stream);
    }
    if (picked) {   // behind either form of the blend: out_depth becomes the picked Gaussian's range, the image buffer's last plane names it
        lg::MedianFwdArgs ma;
        ma.grid = L.grid; ma.ranges = img.ranges; ma.point_list = bin.val_a; ma.rec = geom.rec; ma.rowspan = geom.rowspan;
        ma.coltab = img.coltab; ma.rowtab = img.rowtab; ma.out_depth = out.out_depth; ma.median_id = img.median_id;
        lg::launch_render_picked(ma, mode.depth, mode.return_gap, stream);
        LG_STAGE_CHECK(PICKED_STAGE[(int)mode.depth].check);
        lg::prof_mark(PICKED_STAGE[(int)mode.depth].mark, stream);
    }

    // the selection a backward on these buffers will make (backward_impl starts from the same call): counted now, while the buffers are certainly alive
    const lg::RenderBwdArgs v = backward_selection(L, img, bin);
    lg::note_forward((size_t)P, R, L, geom.totals, ra.flags, geom.touched, (R != 0 && !transmittance_pass) ? &v : nullptr, stream);
    return rendered;
}

// The same for backward_impl: which forward made the buffers (its layout must be carved the same way), what lies behind a shell, the pose form's extras.
struct BackMode {
    bool is_shell = false;                       // the buffers are lidargs_forward_shell*'s
    const float* behind = nullptr;               // shell: the colour / depth sums of the shells behind this one, per pixel
    const float* T_final_global = nullptr;       // shell: the frame's final transmittance, per pixel
    int col_lo = -1, col_hi = -1;                // >= 0: the buffers are a column wedge's
    float* dL_dviewmatrix = nullptr;             // lgpose_backward_view: run the chain's pose form and fold its partial rows into these sixteen
    float* view_partials = nullptr;              // ... through this scratch (lgpose_view_partial_floats)
};

int backward_impl(const SceneArgs sc, const SavedFrame saved, const FrameGrads grads, const BackMode mode, int debug, hipStream_t stream) {
    const int P = sc.P, R = saved.R, width = sc.width, height = sc.height, col_lo = mode.col_lo, col_hi = mode.col_hi;
    const GradRows& rows = grads.rows;
    if (P < 0 || R < 0 || width <= 0 || height <= 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "backward: bad sizes%s");
    if (P == 0) return 0;   // R3/rasterize_points.cu:177
    if (!saved.geom_buffer || !saved.binning_buffer || !saved.image_buffer) return fail(LIDARGS_ERR_STATE, "backward: missing forward buffers%s");
    if (!sc.means3D || !sc.viewmatrix || !saved.radii || !grads.dL_dpix || !grads.dL_dout_depth || !grads.dL_dout_occ || !rows.required(sc.cov3D_precomp))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "backward: NULL required pointer%s");

    lg::GeomView geom; lg::geom_carve(saved.geom_buffer, (size_t)P, lg::GAUSS_BUFFERS, &geom);
    // The accumulation mode is the forward's and travels in the geometry buffer (LG_TOTALS_MODE_WORD); the host never reads it.  On a plain
    // frame's buffers the kernels are handed the word and the place deterministic buffers keep their 64-bit lines at; shell and wedge
    // forwards refuse the mode, so their backwards do not look -- and nobody looks in a process that never made a deterministic forward.
    const bool may_be_det = !mode.is_shell && col_lo < 0 && lg::g_deterministic_seen.load(std::memory_order_relaxed);
    const uint32_t* const det_mode = may_be_det ? geom.totals + LG_TOTALS_MODE_WORD : nullptr;
    // The depth mode travels in the same word (LG_MODE_MEDIAN), under the same rules: only lidargs_forward makes median buffers, and
    // nobody looks before this process has made one.
    const bool may_be_median = !mode.is_shell && col_lo < 0 && lg::g_median_seen.load(std::memory_order_relaxed);
    // a column wedge's buffers: only its own patches were rendered
    if (col_lo >= 0 && (col_lo % LG_TILE_W || col_hi <= col_lo || col_hi > width)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "backward: bad column wedge%s");
    const lg::FrameLayout L = lg::frame_layout(R, width, height, col_lo, col_hi, mode.is_shell ? lg::FRAME_SHELL : lg::FRAME_GAUSS);   // (from the forward's num_rendered)
    lg::BinView bin; L.bin_carve(saved.binning_buffer, &bin);
    lg::ImgView img; lg::img_carve(saved.image_buffer, width, height, lg::make_grid(width, height, 4).num_tiles(), &img);
    lg::prof_begin(stream, 1);

    // Only the Gaussians the forward marked as touched are ever added to, and every backward on these buffers (the first, or a later one
    // under retain_graph) starts by clearing exactly their packed lines, listing them, and zeroing the caller's gradient rows.
    lg::launch_zero_touched(geom.touched, reinterpret_cast<float4*>(geom.gacc), 4, (size_t)P, geom.tlist, geom.tcount, rows.zero_rows(), stream, det_mode, geom.acc64);
    lg::prof_mark("bwd_zero", stream);

    lg::RenderBwdArgs rb = backward_selection(L, img, bin);
    rb.point_list = bin.val_a; rb.rec = geom.rec; rb.rowspan = geom.rowspan; rb.coltab = img.coltab; rb.rowtab = img.rowtab; rb.bg = sc.background; rb.final_T = img.final_T;
    rb.T_final_global = mode.T_final_global; rb.behind = mode.behind;
    rb.dL_dpix = grads.dL_dpix; rb.dL_ddepth = grads.dL_dout_depth; rb.dL_docc = grads.dL_dout_occ; rb.gacc = geom.gacc;
    if (L.work_list) rb.walk = lg::work_list(bin);
    rb.det_mode = (may_be_det || may_be_median) ? geom.totals + LG_TOTALS_MODE_WORD : nullptr;
    rb.acc64 = may_be_det ? geom.acc64 : nullptr;
    lg::launch_render_backward(rb, stream);
    LG_STAGE_CHECK("render backward");
    lg::prof_mark("render_bwd", stream);
    if (may_be_median) {
        // (img.median_id is computed from the default size of the image buffer: on a default buffer it points behind it and is never read)
        lg::MedianBwdArgs mb;
        mb.mode = geom.totals + LG_TOTALS_MODE_WORD; mb.median_id = img.median_id; mb.dL_ddepth = grads.dL_dout_depth; mb.gacc = geom.gacc;
        mb.N = (size_t)width * height; mb.P = (uint32_t)P;
        lg::launch_median_backward(mb, stream);
        LG_STAGE_CHECK("median backward");
        lg::prof_mark("median_bwd", stream);
    }

    lg::GaussBwdArgs gb = gauss_bwd_args(sc, rows, geom.gacc, geom.tlist, geom.tcount);
    gb.radii = saved.radii; gb.det_mode = det_mode; gb.acc64 = geom.acc64;
    if (mode.dL_dviewmatrix) {   // lgpose_backward_view: the chain's pose form and the fold of its partial rows (two launches for one)
        gb.view_partials = mode.view_partials;
        lg::launch_gaussian_backward_view(gb, mode.dL_dviewmatrix, stream);
    } else lg::launch_gaussian_backward(gb, stream);
    LG_STAGE_CHECK("gaussian backward");
    lg::prof_mark("gaussian_bwd", stream);
    return 0;
}

}  // namespace

// The C parameter lists onto the argument structs.  The six 3-D forwards spell their common parameters with the same names, and so do the four backwards:
// each mapping is written once, as a macro because only the preprocessor can take a name from the entry point it is used in.  Every field is bound BY NAME.
#define LG_FORWARD_ARGS(alloc, sc, out)                                                                                                                                                     \
    FrameAllocs alloc; SceneArgs sc; FrameOutputs out;                                                                                                                                      \
    alloc.geometry = geometry_alloc; alloc.geometry_user = geometry_user; alloc.binning = binning_alloc; alloc.binning_user = binning_user; alloc.image = image_alloc; alloc.image_user = image_user;\
    sc.P = P; sc.width = width; sc.height = height; sc.background = background; sc.means3D = means3D; sc.colors_precomp = colors_precomp; sc.opacities = opacities; sc.scales = scales;     \
    sc.scale_modifier = scale_modifier; sc.rotations = rotations; sc.cov3D_precomp = cov3D_precomp; sc.viewmatrix = viewmatrix; sc.beams = beam_inclinations;                               \
    sc.near_f = (float)lidar_near; sc.far_f = (float)lidar_far;                                                                                                                             \
    out.out_color = out_color; out.out_depth = out_depth; out.out_occ = out_occ; out.radii = radii; out.radii_xy = radii_xy
// What the chain reads of the scene (the backwards and the chain's two test hooks); the seven rows every one of them has; the five scratch rows lidargs_backward_wedge lacks.
#define LG_CHAIN_SCENE(sc)                                                                                                                                                                  \
    sc.P = P; sc.means3D = means3D; sc.scales = scales; sc.scale_modifier = scale_modifier; sc.rotations = rotations; sc.cov3D_precomp = cov3D_precomp; sc.viewmatrix = viewmatrix
#define LG_GRAD_ROWS(rows)                                                                                                                                                                  \
    rows.dL_dmean2D = dL_dmean2D; rows.dL_dopacity = dL_dopacity; rows.dL_dcolor = dL_dcolor; rows.dL_dmean3D = dL_dmean3D; rows.dL_dcov3D = dL_dcov3D; rows.dL_dscale = dL_dscale; rows.dL_drot = dL_drot
#define LG_SCRATCH_ROWS(rows)                                                                                                                                                               \
    rows.dL_dconic = dL_dconic; rows.dL_ddepths = dL_ddepths; rows.dL_dsphere_means3D = dL_dsphere_means3D; rows.dL_dbasis_u1 = dL_dbasis_u1; rows.dL_dbasis_u2 = dL_dbasis_u2
#define LG_BACKWARD_ARGS(sc, saved, grads)                                                                                                                                                  \
    SceneArgs sc; SavedFrame saved; FrameGrads grads;                                                                                                                                       \
    LG_CHAIN_SCENE(sc); sc.width = width; sc.height = height; sc.background = background;                                                                                                   \
    saved.R = R; saved.radii = radii; saved.geom_buffer = geom_buffer; saved.binning_buffer = binning_buffer; saved.image_buffer = image_buffer;                                            \
    grads.dL_dpix = dL_dpix; grads.dL_dout_depth = dL_dout_depth; grads.dL_dout_occ = dL_dout_occ; LG_GRAD_ROWS(grads.rows)
extern "C" {

int lidargs_abi_version(void) { return LIDARGS_ABI_VERSION; }
const char* lidargs_last_error(void) { return g_err; }

int lidargs_forward(lidargs_alloc_fn geometry_alloc, void* geometry_user, lidargs_alloc_fn binning_alloc, void* binning_user,
                    lidargs_alloc_fn image_alloc, void* image_user, int P, int D, int M, const float* background, int width,
                    int height, const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const float* beam_inclinations,
                    int prefiltered, int lidar_far, int lidar_near, float* out_color, float* out_depth, float* out_occ,
                    int* radii, int* radii_xy, int debug, void* stream) {
    (void)D; (void)M; (void)shs; (void)projmatrix; (void)cam_pos; (void)prefiltered;
    FrameMode mode;
    mode.deterministic = lg::deterministic_requested();
    mode.depth = lg::depth_mode();
    if (mode.depth == lg::DepthMode::Second) mode.return_gap = lg::return_gap();
    if (mode.deterministic && lg::picked(mode.depth))   // (a picked Gaussian's depth gradient is added with a float atomic: not what the other switch promises)
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "%s: a non-default LIDARGS_DEPTH (" LG_PICKED_DEPTH_NAMES ") is not supported together with LIDARGS_DETERMINISTIC=1; unset one of them for this call", "lidargs_forward");
    LG_FORWARD_ARGS(alloc, sc, out);
    return forward_impl(alloc, sc, out, mode, debug, (hipStream_t)stream);
}

int lidargs_forward_enqueue(lidargs_alloc_fn geometry_alloc, void* geometry_user, lidargs_alloc_fn binning_alloc, void* binning_user,
                            lidargs_alloc_fn image_alloc, void* image_user, int P, int D, int M, const float* background, int width,
                            int height, const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                            const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                            const float* viewmatrix, const float* projmatrix, const float* cam_pos, const float* beam_inclinations,
                            int prefiltered, int lidar_far, int lidar_near, float* out_color, float* out_depth, float* out_occ,
                            int* radii, int* radii_xy, int debug, int instance_capacity, int tile_rows, unsigned* status_host, void* stream) {
    (void)D; (void)M; (void)shs; (void)projmatrix; (void)cam_pos; (void)prefiltered;
    if (const int rc = lg::refuse_modes("lidargs_forward_enqueue")) return rc;
    if (instance_capacity <= 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward_enqueue: instance_capacity must be positive%s");
    FrameMode mode;
    mode.instance_capacity = instance_capacity; mode.fixed_tile_rows = tile_rows; mode.status_host = status_host;
    LG_FORWARD_ARGS(alloc, sc, out);
    return forward_impl(alloc, sc, out, mode, debug, (hipStream_t)stream);
}

int lidargs_backward(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                     const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                     const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                     const float* campos, const float* beam_inclinations, float tan_fovx, float tan_fovy, const int* radii,
                     char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix,
                     const float* dL_dout_depth, const float* dL_dout_occ, float* dL_dmean2D, float* dL_dconic,
                     float* dL_dopacity, float* dL_dcolor, float* dL_ddepths, float* dL_dmean3D, float* dL_dsphere_means3D,
                     float* dL_dbasis_u1, float* dL_dbasis_u2, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                     int debug, void* stream) {
    (void)D; (void)M; (void)shs; (void)colors_precomp; (void)projmatrix; (void)campos; (void)beam_inclinations; (void)tan_fovx; (void)tan_fovy; (void)dL_dsh;
    LG_BACKWARD_ARGS(sc, saved, grads); LG_SCRATCH_ROWS(grads.rows);
    return backward_impl(sc, saved, grads, BackMode(), debug, (hipStream_t)stream);
}

size_t lgpose_view_partial_floats(int P) { return lg::view_partial_floats(P); }

int lgpose_backward_view(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                          const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                          const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                          const float* campos, const float* beam_inclinations, float tan_fovx, float tan_fovy, const int* radii,
                          char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix,
                          const float* dL_dout_depth, const float* dL_dout_occ, float* dL_dmean2D, float* dL_dconic,
                          float* dL_dopacity, float* dL_dcolor, float* dL_ddepths, float* dL_dmean3D, float* dL_dsphere_means3D,
                          float* dL_dbasis_u1, float* dL_dbasis_u2, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                          int debug, void* stream, float* dL_dviewmatrix, float* view_partials, size_t view_partial_floats) {
    (void)D; (void)M; (void)shs; (void)colors_precomp; (void)projmatrix; (void)campos; (void)beam_inclinations; (void)tan_fovx; (void)tan_fovy; (void)dL_dsh;
    if (P < 0 || R < 0 || width <= 0 || height <= 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "backward_view: bad sizes%s");
    if (!dL_dviewmatrix) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "backward_view: dL_dviewmatrix is NULL%s");
    if (P == 0) {   // lidargs_backward's early return, and the sixteen zeros
        LG_HIP(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float), (hipStream_t)stream));
        return 0;
    }
    if (!view_partials || ((uintptr_t)view_partials & 15u) || view_partial_floats < lg::view_partial_floats(P))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "backward_view: view_partials is NULL, not 16-byte aligned or shorter than lgpose_view_partial_floats(P)%s");
    BackMode mode; mode.dL_dviewmatrix = dL_dviewmatrix; mode.view_partials = view_partials;
    LG_BACKWARD_ARGS(sc, saved, grads); LG_SCRATCH_ROWS(grads.rows);
    return backward_impl(sc, saved, grads, mode, debug, (hipStream_t)stream);
}

int lidargs_visible_filter(lidargs_alloc_fn geometry_alloc, void* geometry_user, lidargs_alloc_fn binning_alloc, void* binning_user,
                           lidargs_alloc_fn image_alloc, void* image_user, int P, int M, int width, int height,
                           const float* means3D, const float* scales, float scale_modifier, const float* rotations,
                           const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                           const float* beam_inclinations, float tan_fovx, float tan_fovy, int prefiltered, int lidar_far,
                           int lidar_near, int* radii, int* radii_xy, int debug, void* stream_) {
    (void)geometry_alloc; (void)geometry_user; (void)binning_alloc; (void)binning_user; (void)image_alloc; (void)image_user;
    (void)M; (void)projmatrix; (void)cam_pos; (void)tan_fovx; (void)tan_fovy; (void)prefiltered;
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || width <= 0 || height < 2) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "visible_filter: bad sizes%s");
    if (P == 0) return 0;
    if (!means3D || !viewmatrix || !beam_inclinations || !radii)   // radii_xy: optional
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "visible_filter: NULL required pointer%s");
    if (!cov3D_precomp && (!scales || !rotations)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "visible_filter: need scales+rotations or cov3D_precomp%s");
    const lg::TileGrid grid = lg::make_grid(width, height, lg::tile_rows());
    const float inf = std::numeric_limits<float>::infinity();
    const lg::PreprocessParams pp = preprocess_params(P, grid, scale_modifier, (float)lidar_near, (float)lidar_far, -inf, inf, viewmatrix);
    lg::GeomView none; memset(&none, 0, sizeof none);
    lg::launch_preprocess(pp, means3D, scales, rotations, nullptr, nullptr, cov3D_precomp, beam_inclinations, radii, radii_xy, none,
                          nullptr, true, stream);
    LG_STAGE_CHECK("filter preprocess");
    return 0;
}

int lidargs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, unsigned char* present,
                         void* stream_) {
    (void)projmatrix;
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (P < 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "mark_visible: bad size%s");
    if (P == 0) return 0;
    if (!means3D || !viewmatrix || !present) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "mark_visible: NULL required pointer%s");
    lg::launch_mark_visible(P, means3D, viewmatrix, present, stream);
    LG_STAGE_CHECK("mark visible");
    return 0;
}

int lidargs_debug_rects(int n, int surfel, const float* p_cr, const int* r_xy, int tiles_x, int tiles_y, int* rects, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (n < 0 || tiles_x < 0 || tiles_y < 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_rects: bad size%s");
    if (n == 0) return 0;
    if (!p_cr || !r_xy || !rects) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_rects: NULL required pointer%s");
    lg::launch_debug_rects(n, surfel, p_cr, r_xy, tiles_x, tiles_y, rects, stream);
    LG_STAGE_CHECK("debug rects");
    return 0;
}

// Test hooks of the sorts (binning.hip): the product's own launchers on caller-supplied pairs; no dispatch is decided here.
size_t lidargs_debug_sort_scratch_words(size_t n, int scratch_bits) {
    if (scratch_bits < 1 || scratch_bits > lg::SORT_MAX_RADIX_BITS) scratch_bits = lg::SORT_RADIX_BITS;
    return lg::sort_scratch_words(n, scratch_bits);
}

int lidargs_debug_sort_result_side(size_t n, int end_bit) { return lg::radix_sort_result_side(n, end_bit); }

int lidargs_debug_sort_pairs(size_t n, int key_bytes, void* key_a, void* key_b, unsigned* val_a, unsigned* val_b, int begin_bit, int end_bit,
                             int max_bits, int scratch_bits, unsigned* scratch, const unsigned* n_dev, int vals_are_positions, int bias_on,
                             size_t kmin, size_t cull, int tail_mode, const void* tail_src, void* tail_dst, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (key_bytes != 2 && key_bytes != 4) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_sort_pairs: key_bytes must be 2 or 4%s");
    if (n > (size_t)std::numeric_limits<int>::max()) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_sort_pairs: bad size%s");
    if (begin_bit < 0 || end_bit < begin_bit || end_bit > 8 * key_bytes) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_sort_pairs: bad bit range%s");
    if (max_bits < 0 || max_bits > lg::SORT_MAX_RADIX_BITS) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_sort_pairs: bad digit width%s");
    const int digit = max_bits ? max_bits : lg::SORT_RADIX_BITS;
    if (scratch_bits != 0 && (scratch_bits < digit || scratch_bits > lg::SORT_MAX_RADIX_BITS))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_sort_pairs: scratch_bits must be 0 or in [digit width, 11]%s");
    if (tail_mode < 0 || tail_mode > 2 || (tail_mode != 0 && (!tail_src || !tail_dst)))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_sort_pairs: bad tail%s");
    if (kmin > 0xFFFFFFFFull || cull > 0xFFFFFFFFull) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_sort_pairs: the bias is 32 bits wide%s");
    if (key_bytes == 2 && (tail_mode != 0 || bias_on || begin_bit != 0 || vals_are_positions || scratch_bits != 0 || digit != lg::SORT_RADIX_BITS))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_sort_pairs: 16-bit keys have no tail, bias, begin_bit, positions or other digit width%s");
    if (n == 0) return 0;
    if (!key_a || !key_b || !val_b || !scratch || (!val_a && !vals_are_positions))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_sort_pairs: NULL required pointer%s");
    int side;
    if (key_bytes == 2) {
        side = lg::launch_radix_sort_pairs16(static_cast<uint16_t*>(key_a), static_cast<uint16_t*>(key_b), val_a, val_b, n, end_bit, scratch, stream, n_dev);
    } else {
        lg::RadixTail tail; tail.src = tail_src; tail.dst = tail_dst; tail.mode = tail_mode;
        lg::KeyBias kb; kb.kmin = (uint32_t)kmin; kb.cull = (uint32_t)cull;
        side = lg::launch_radix_sort_pairs(static_cast<uint32_t*>(key_a), static_cast<uint32_t*>(key_b), val_a, val_b, n, end_bit, scratch, stream, max_bits,
                                           n_dev, scratch_bits, vals_are_positions != 0, tail, begin_bit, bias_on ? &kb : nullptr);
    }
    LG_STAGE_CHECK("debug sort pairs");
    return side;
}

int lidargs_debug_range_sort_rest(size_t key_min, size_t key_max, unsigned* plan) {
    if (!plan || key_min > 0xFFFFFFFFull || key_max > 0xFFFFFFFFull) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_range_sort_rest: bad argument%s");
    const lg::RangeSortRest r = lg::range_sort_rest(~(uint32_t)key_min, (uint32_t)key_max);
    plan[0] = r.bias.kmin; plan[1] = r.bias.cull; plan[2] = (unsigned)r.end_bit; plan[3] = (unsigned)r.max_bits;
    return 0;
}

int lidargs_debug_range_sort_buckets(size_t P, unsigned* key_a, unsigned* key_b, unsigned* id_a, unsigned* id_b, unsigned* scratch,
                                     const unsigned* key_span, int tail_mode, const void* tail_src, void* tail_dst, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (P > (size_t)std::numeric_limits<int>::max()) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_range_sort_buckets: bad size%s");
    if (!lg::range_sort_buckets_ok(P)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_range_sort_buckets: no frame of this size takes the bucketed form%s");
    if (tail_mode < 1 || tail_mode > 2) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_range_sort_buckets: tail_mode must be 1 or 2%s");
    if (!key_a || !key_b || !id_a || !id_b || !scratch || !key_span || !tail_src || !tail_dst)
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_range_sort_buckets: NULL required pointer%s");
    lg::RadixTail tail; tail.src = tail_src; tail.dst = tail_dst; tail.mode = tail_mode;
    lg::launch_range_sort_buckets(key_a, key_b, id_a, id_b, P, scratch, key_span, tail, stream);
    LG_STAGE_CHECK("debug range sort buckets");
    return 0;
}

// Test hooks of the scan, the instance emit and the tile ranges (binning.hip): the product's own launchers on caller-supplied arrays.
size_t lidargs_debug_scan_scratch_words(size_t n) { return lg::scan_scratch_words(n); }

int lidargs_debug_exclusive_scan(size_t n, const unsigned* in, unsigned* out, unsigned* total_out, unsigned* scratch, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (n > (size_t)std::numeric_limits<int>::max()) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_exclusive_scan: bad size%s");
    if (n != 0 && (!in || !out || !scratch)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_exclusive_scan: NULL required pointer%s");
    lg::launch_exclusive_scan(in, out, n, total_out, scratch, stream);
    LG_STAGE_CHECK("debug exclusive scan");
    return 0;
}

int lidargs_debug_emit_instances(size_t P, int compact, int tile_rows, int tiles_x, int tiles_y, const unsigned* ids_sorted, const void* span_sorted,
                                 unsigned* block_off, unsigned* total_out, int scan_block_sums, int key_bytes, void* inst_tile, unsigned* inst_val,
                                 size_t cap, unsigned* ranges, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (!(tile_rows == 4 || tile_rows == 8 || tile_rows == 16 || tile_rows == 32))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_emit_instances: tile_rows must be 4, 8, 16 or 32%s");
    if (key_bytes != 2 && key_bytes != 4) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_emit_instances: key_bytes must be 2 or 4%s");
    if (tiles_x <= 0 || tiles_y <= 0 || (long long)tiles_x * tiles_y > (long long)std::numeric_limits<int>::max())
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_emit_instances: bad grid%s");
    if (key_bytes == 2 && (long long)tiles_x * tiles_y > 65536) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_emit_instances: 16-bit keys hold at most 65536 tiles%s");
    if (compact && tiles_x > 256) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_emit_instances: compact records hold at most 256 tile columns%s");
    if (P > (size_t)std::numeric_limits<int>::max() || cap > 0xFFFFFFFFull) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_emit_instances: bad size%s");
    if (P == 0) return 0;                                              // (the launchers would ask for a grid of zero blocks)
    if (!ids_sorted || !span_sorted || !block_off || !inst_tile || !inst_val || (scan_block_sums && !total_out))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_emit_instances: NULL required pointer%s");
    lg::TileGrid grid{};
    grid.TH = tile_rows; grid.tiles_x = grid.ref_tiles_x = grid.x_n = tiles_x; grid.tiles_y = tiles_y;
    grid.W = 16 * tiles_x; grid.H = tile_rows * tiles_y; grid.waves_per_tile = 1;
    lg::launch_instance_offsets(span_sorted, compact != 0, tile_rows, block_off, total_out, P, stream, scan_block_sums != 0);
    LG_STAGE_CHECK("debug instance offsets");
    lg::launch_emit_instances(ids_sorted, block_off, span_sorted, compact != 0, P, grid, static_cast<uint32_t*>(inst_tile), inst_val, stream, (uint32_t)cap,
                              key_bytes == 2, reinterpret_cast<uint2*>(ranges), scan_block_sums == 0);
    LG_STAGE_CHECK("debug emit instances");
    return 0;
}

int lidargs_debug_tile_ranges(size_t R, int key_bytes, const void* tile_sorted, const unsigned* R_dev, unsigned* ranges, int tiles, unsigned* zero,
                              int n_zero, int prezeroed, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (key_bytes != 2 && key_bytes != 4) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_tile_ranges: key_bytes must be 2 or 4%s");
    if (R > (size_t)std::numeric_limits<int>::max() || tiles < 0 || n_zero < 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_tile_ranges: bad size%s");
    if (key_bytes == 2 && tiles > 65536) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_tile_ranges: 16-bit keys hold at most 65536 tiles%s");
    if ((tiles && !ranges) || (R && !tile_sorted)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_tile_ranges: NULL required pointer%s");
    if (reinterpret_cast<uintptr_t>(tile_sorted) & 15u) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_tile_ranges: tile_sorted must be 16-byte aligned%s");
    lg::launch_tile_ranges(static_cast<const uint32_t*>(tile_sorted), R, reinterpret_cast<uint2*>(ranges), tiles, stream, R_dev, key_bytes == 2, zero, n_zero,
                           prezeroed != 0);
    LG_STAGE_CHECK("debug tile ranges");
    return 0;
}

// Test hooks of the two per-Gaussian stages (preprocess.hip): the product's own launchers on caller-supplied arrays; no dispatch is decided here.
int lidargs_debug_preprocess(int P, int width, int height, const float* means3D, const float* colors, const float* opacities, const float* scales,
                             float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* beams,
                             float near_f, float far_f, float shell_lo, float shell_hi, int tile_x_lo, int tile_x_hi, int compact, int prune,
                             const unsigned* n_valid, float* rec, unsigned* rowspan, unsigned* spans, unsigned* key, unsigned char* touched,
                             unsigned* totals, int* radii, int* radii_xy, float* coltab, float* rowtab, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (P < 0 || width <= 0 || height < 2 || height > 65535 || width > 65535 * 16) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_preprocess: bad sizes%s");
    const lg::TileGrid grid4 = lg::make_grid(width, height, 4);
    if (tile_x_lo < 0 || tile_x_hi <= tile_x_lo || tile_x_hi > grid4.tiles_x) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_preprocess: the tile-column window lies outside the grid%s");
    if (compact && !lg::compact_spans(grid4.tiles_x, height)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_preprocess: compact span records do not hold this image%s");
    if (!means3D || !colors || !opacities || !viewmatrix || !beams || !rec || !rowspan || !spans || !key || !touched || !totals || !radii)   // radii_xy: optional
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_preprocess: NULL required pointer%s");
    if (!cov3D_precomp && (!scales || !rotations)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_preprocess: need scales+rotations or cov3D_precomp%s");
    if ((coltab == nullptr) != (rowtab == nullptr)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_preprocess: the two ray tables come together%s");
    if (P == 0) return 0;
    lg::PreprocessParams pp = preprocess_params(P, grid4, scale_modifier, near_f, far_f, shell_lo, shell_hi, viewmatrix);
    pp.tile_x_lo = tile_x_lo; pp.tile_x_hi = tile_x_hi; pp.compact = compact ? 1 : 0; pp.prune = prune ? 1 : 0; pp.n_valid = n_valid;
    lg::GeomView geom; memset(&geom, 0, sizeof geom);
    geom.rec = reinterpret_cast<float4*>(rec); geom.rowspan = rowspan; geom.spans = reinterpret_cast<uint4*>(spans); geom.key_a = key;
    geom.touched = touched; geom.totals = totals;
    lg::ImgView img; memset(&img, 0, sizeof img);
    img.coltab = reinterpret_cast<float2*>(coltab); img.rowtab = reinterpret_cast<float2*>(rowtab);
    LG_HIP(hipMemsetAsync(totals, 0, LG_TOTALS_WORDS * sizeof(uint32_t), stream));     // as forward_impl does
    lg::launch_preprocess(pp, means3D, scales, rotations, opacities, colors, cov3D_precomp, beams, radii, radii_xy, geom, coltab ? &img : nullptr, false, stream);
    LG_STAGE_CHECK("debug preprocess");
    return 0;
}

int lidargs_debug_gaussian_backward(int P, int line_f4, int stage, const unsigned char* touched, float* gacc, const float* means3D,
                                    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                    const float* viewmatrix, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                                    float* dL_ddepths, float* dL_dmean3D, float* dL_dsphere_means3D, float* dL_dbasis_u1, float* dL_dbasis_u2,
                                    float* dL_dcov3D, float* dL_dscale, float* dL_drot, unsigned char* tlist, unsigned short* tcount, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (P < 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_gaussian_backward: bad size%s");
    if (line_f4 != 4 && line_f4 != 8) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_gaussian_backward: line_f4 must be 4 or 8%s");
    if (stage < 0 || stage > 2 || (line_f4 == 8 && stage != 1)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_gaussian_backward: stage must be 0, 1 or 2, and 1 for the surfel line%s");
    if (!touched || !gacc || !tlist || !tcount) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_gaussian_backward: NULL required pointer%s");
    const bool chain = stage != 1;
    SceneArgs sc; GradRows rows; LG_CHAIN_SCENE(sc); LG_GRAD_ROWS(rows); LG_SCRATCH_ROWS(rows);
    // the chain's rows, as backward_impl requires them (dL_dconic, dL_ddepths, dL_dsphere_means3D, dL_dbasis_u1/u2 stay optional)
    if (chain && (!means3D || !viewmatrix || !rows.required(cov3D_precomp)))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_gaussian_backward: NULL required pointer%s");
    if (chain && !cov3D_precomp && (!scales || !rotations)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_gaussian_backward: need scales+rotations or cov3D_precomp%s");
    if (P == 0) return 0;
    if (stage != 2) {
        lg::launch_zero_touched(touched, reinterpret_cast<float4*>(gacc), line_f4, (size_t)P, tlist, tcount, rows.zero_rows(), stream);
        LG_STAGE_CHECK("debug zero touched");
    }
    if (!chain) return 0;
    lg::GaussBwdArgs gb = gauss_bwd_args(sc, rows, gacc, tlist, tcount); gb.radii = nullptr;
    lg::launch_gaussian_backward(gb, stream);
    LG_STAGE_CHECK("debug gaussian backward");
    return 0;
}

int lgpose_debug_view_backward(int P, const float* gacc, const float* means3D, const float* scales, float scale_modifier, const float* rotations,
                                const float* cov3D_precomp, const float* viewmatrix, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                                float* dL_dcolor, float* dL_ddepths, float* dL_dmean3D, float* dL_dsphere_means3D, float* dL_dbasis_u1,
                                float* dL_dbasis_u2, float* dL_dcov3D, float* dL_dscale, float* dL_drot, const unsigned char* tlist,
                                const unsigned short* tcount, const unsigned* mode_word, const long long* acc64, float* dL_dviewmatrix,
                                float* view_partials, size_t view_partial_floats, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (P < 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_view_backward: bad size%s");
    if (!dL_dviewmatrix) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_view_backward: dL_dviewmatrix is NULL%s");
    if (P == 0) {
        LG_HIP(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float), stream));
        return 0;
    }
    if (!view_partials || ((uintptr_t)view_partials & 15u) || view_partial_floats < lg::view_partial_floats(P))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_view_backward: view_partials is NULL, not 16-byte aligned or shorter than lgpose_view_partial_floats(P)%s");
    SceneArgs sc; GradRows rows; LG_CHAIN_SCENE(sc); LG_GRAD_ROWS(rows); LG_SCRATCH_ROWS(rows);
    if (!gacc || !tlist || !tcount || !means3D || !viewmatrix || !rows.required(cov3D_precomp) || ((mode_word == nullptr) != (acc64 == nullptr)))
        return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_view_backward: NULL required pointer%s");
    if (!cov3D_precomp && (!scales || !rotations)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_view_backward: need scales+rotations or cov3D_precomp%s");
    lg::GaussBwdArgs gb = gauss_bwd_args(sc, rows, gacc, tlist, tcount); gb.radii = nullptr; gb.det_mode = mode_word; gb.acc64 = acc64;
    gb.view_partials = view_partials;
    lg::launch_gaussian_backward_view(gb, dL_dviewmatrix, stream);
    LG_STAGE_CHECK("debug view backward");
    return 0;
}

int lidargs_forward_shell(lidargs_alloc_fn geometry_alloc, void* geometry_user, lidargs_alloc_fn binning_alloc, void* binning_user,
                          lidargs_alloc_fn image_alloc, void* image_user, int P, const float* background, int width, int height,
                          const float* means3D, const float* colors_precomp, const float* opacities, const float* scales,
                          float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                          const float* beam_inclinations, int lidar_far, int lidar_near, float shell_lo, float shell_hi,
                          const float* T_in, int transmittance_pass, float* out_color, float* out_depth, float* out_occ,
                          float* T_out, int* radii, int* radii_xy, int debug, void* stream) {
    if (const int rc = lg::refuse_modes("lidargs_forward_shell")) return rc;
    FrameMode mode;
    mode.is_shell = true; mode.shell_lo = shell_lo; mode.shell_hi = shell_hi;
    mode.T_in = T_in; mode.transmittance_pass = transmittance_pass; mode.T_out = T_out;
    LG_FORWARD_ARGS(alloc, sc, out);
    return forward_impl(alloc, sc, out, mode, debug, (hipStream_t)stream);
}

int lidargs_forward_shell_enqueue(lidargs_alloc_fn geometry_alloc, void* geometry_user, lidargs_alloc_fn binning_alloc, void* binning_user,
                                  lidargs_alloc_fn image_alloc, void* image_user, int P, const float* background, int width, int height,
                                  const float* means3D, const float* colors_precomp, const float* opacities, const float* scales,
                                  float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                  const float* beam_inclinations, int lidar_far, int lidar_near, float shell_lo, float shell_hi,
                                  const float* T_in, int transmittance_pass, float* out_color, float* out_depth, float* out_occ,
                                  float* T_out, int* radii, int* radii_xy, int debug, const unsigned* n_valid, int instance_capacity,
                                  int tile_rows, unsigned* status_host, void* stream) {
    if (const int rc = lg::refuse_modes("lidargs_forward_shell_enqueue")) return rc;
    if (instance_capacity <= 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward_shell_enqueue: instance_capacity must be positive%s");
    FrameMode mode;
    mode.is_shell = true; mode.shell_lo = shell_lo; mode.shell_hi = shell_hi; mode.n_valid = n_valid;
    mode.T_in = T_in; mode.transmittance_pass = transmittance_pass; mode.T_out = T_out;
    mode.instance_capacity = instance_capacity; mode.fixed_tile_rows = tile_rows; mode.status_host = status_host;
    LG_FORWARD_ARGS(alloc, sc, out);
    return forward_impl(alloc, sc, out, mode, debug, (hipStream_t)stream);
}

// ---- column wedges (multi-GPU): rank g bins and renders the tile columns of pixel columns [col_lo, col_hi) only --------------------
int lidargs_forward_wedge(lidargs_alloc_fn geometry_alloc, void* geometry_user, lidargs_alloc_fn binning_alloc, void* binning_user,
                          lidargs_alloc_fn image_alloc, void* image_user, int P, const float* background, int width, int height,
                          const float* means3D, const float* colors_precomp, const float* opacities, const float* scales,
                          float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                          const float* beam_inclinations, int lidar_far, int lidar_near, int col_lo, int col_hi, float* out_color,
                          float* out_depth, float* out_occ, int* radii, int* radii_xy, int debug, void* stream) {
    if (const int rc = lg::refuse_modes("lidargs_forward_wedge")) return rc;
    if (col_lo < 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward_wedge: col_lo < 0%s");
    // lidargs_wedge_select_count bounds a Gaussian's reach from its scales and rotation; a precomputed covariance has no such bound
    // there, and a wedge rendered from an under-selected set would silently miss its boundary Gaussians
    if (cov3D_precomp) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward_wedge: cov3D_precomp is not supported on the column-wedge path (give scales + rotations)%s");
    FrameMode mode;
    mode.col_lo = col_lo; mode.col_hi = col_hi;
    LG_FORWARD_ARGS(alloc, sc, out);
    return forward_impl(alloc, sc, out, mode, debug, (hipStream_t)stream);
}

int lidargs_forward_wedge_enqueue(lidargs_alloc_fn geometry_alloc, void* geometry_user, lidargs_alloc_fn binning_alloc, void* binning_user,
                                  lidargs_alloc_fn image_alloc, void* image_user, int P, const float* background, int width, int height,
                                  const float* means3D, const float* colors_precomp, const float* opacities, const float* scales,
                                  float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                  const float* beam_inclinations, int lidar_far, int lidar_near, int col_lo, int col_hi, float* out_color,
                                  float* out_depth, float* out_occ, int* radii, int* radii_xy, int debug, const unsigned* n_valid,
                                  int instance_capacity, int tile_rows, unsigned* status_host, void* stream) {
    if (const int rc = lg::refuse_modes("lidargs_forward_wedge_enqueue")) return rc;
    if (col_lo < 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward_wedge: col_lo < 0%s");
    if (cov3D_precomp) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward_wedge: cov3D_precomp is not supported on the column-wedge path (give scales + rotations)%s");
    if (instance_capacity <= 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "forward_wedge_enqueue: instance_capacity must be positive%s");
    FrameMode mode;
    mode.col_lo = col_lo; mode.col_hi = col_hi; mode.n_valid = n_valid;
    mode.instance_capacity = instance_capacity; mode.fixed_tile_rows = tile_rows; mode.status_host = status_host;
    LG_FORWARD_ARGS(alloc, sc, out);
    return forward_impl(alloc, sc, out, mode, debug, (hipStream_t)stream);
}

int lidargs_backward_wedge(int P, int R, const float* background, int width, int height, const float* means3D, const float* colors_precomp,
                           const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                           const float* beam_inclinations, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                           int col_lo, int col_hi, const float* dL_dpix, const float* dL_dout_depth, const float* dL_dout_occ, float* dL_dmean2D,
                           float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dscale, float* dL_drot, int debug,
                           void* stream) {
    if (col_lo < 0) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "backward_wedge: col_lo < 0%s");
    if (cov3D_precomp) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "backward_wedge: cov3D_precomp is not supported on the column-wedge path (give scales + rotations)%s");
    BackMode mode;
    mode.col_lo = col_lo; mode.col_hi = col_hi;
    LG_BACKWARD_ARGS(sc, saved, grads);          // (no scratch rows on this entry point)
    return backward_impl(sc, saved, grads, mode, debug, (hipStream_t)stream);
}

int lidargs_render_shell(int P, int R, const float* background, int width, int height, char* geom_buffer, char* binning_buffer,
                         char* image_buffer, const float* T_in, int transmittance_pass, float* out_color, float* out_depth,
                         float* out_occ, float* T_out, float* T_end_out, int debug, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (P <= 0 || R < 0 || !geom_buffer || !binning_buffer || !image_buffer) return fail(LIDARGS_ERR_STATE, "render_shell: missing forward buffers%s");
    lg::GeomView geom; lg::geom_carve(geom_buffer, (size_t)P, lg::GAUSS_BUFFERS, &geom);
    const lg::FrameLayout L = lg::frame_layout(R, width, height, -1, -1, lg::FRAME_SHELL);
    lg::BinView bin; L.bin_carve(binning_buffer, &bin);
    lg::ImgView img; lg::img_carve(image_buffer, width, height, lg::make_grid(width, height, 4).num_tiles(), &img);
    FrameOutputs out; out.out_color = out_color; out.out_depth = out_depth; out.out_occ = out_occ;
    lg::RenderFwdArgs ra = render_fwd_args(L, geom, bin, img, background, out);   // (touched: a repeated T-only pass sets the same marks again)
    ra.fill.cnt = nullptr;                       // a shell's backward keeps the slot grid
    ra.T_in = T_in; ra.T_pass = T_out; ra.transmittance_only = transmittance_pass;
    ra.alive = L.gated ? bin.alive : nullptr;    // written, like the flags, by the shell's phase 1
    ra.flags = bin.flags;                        // written by the shell's phase 1 (lidargs_forward_shell)
    ra.run_pass1 = transmittance_pass ? 1 : 0;   // phase 2 reuses the Tpass planes the shell's phase 1 left behind
    ra.T_end_out = transmittance_pass ? nullptr : T_end_out;          // the combine writes it beside final_T
    if (!transmittance_pass && (!out_color || !out_depth || !out_occ)) return fail(LIDARGS_ERR_INVALID_ARGUMENT, "render_shell: NULL output%s");
    if (ra.run_pass1) run_pass1_rounds(ra, L.plan, bin.alive, stream);
    if (!transmittance_pass) lg::launch_render_pass2(ra, stream);
    lg::launch_render_combine(ra, stream);
    LG_STAGE_CHECK("render shell");
    return 0;
}

int lidargs_backward_shell(int P, int R, const float* background, int width, int height, const float* means3D,
                           const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                           const float* cov3D_precomp, const float* viewmatrix, const float* beam_inclinations, const int* radii,
                           char* geom_buffer, char* binning_buffer, char* image_buffer, const float* behind,
                           const float* T_final_global, const float* dL_dpix, const float* dL_dout_depth, const float* dL_dout_occ,
                           float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_ddepths,
                           float* dL_dmean3D, float* dL_dsphere_means3D, float* dL_dbasis_u1, float* dL_dbasis_u2,
                           float* dL_dcov3D, float* dL_dscale, float* dL_drot, int debug, void* stream) {
    BackMode mode;
    mode.is_shell = true; mode.behind = behind; mode.T_final_global = T_final_global;
    LG_BACKWARD_ARGS(sc, saved, grads); LG_SCRATCH_ROWS(grads.rows);
    return backward_impl(sc, saved, grads, mode, debug, (hipStream_t)stream);
}

void lidargs_profile_enable(int on) {
    if (on) {
        // create every event up front so that the timed region only pays for hipEventRecord
        if (!g_prof.calls) g_prof.calls = new Profiler::Call[Profiler::MAX_CALLS];
        for (int i = 0; i < Profiler::MAX_CALLS; i++) {
            Profiler::Call& c = g_prof.calls[i];
            if (!c.created) { for (auto& e : c.ev) (void)hipEventCreate(&e); c.created = true; }
            c.n = 0;
        }
        g_prof.ncalls = 0;
        g_prof.seen[0] = g_prof.seen[1] = 0;
        g_prof.every = on > 1 ? on : 1;
    }
    g_prof.enabled = on != 0;
}

// stages of the most recent recorded call
int lidargs_profile_read(float* ms_out, int max_stages) {
    if (!g_prof.calls || g_prof.ncalls == 0) return 0;
    Profiler::Call& c = g_prof.calls[(g_prof.ncalls - 1) % Profiler::MAX_CALLS];
    if (c.n == 0) return 0;
    (void)hipEventSynchronize(c.ev[c.n]);
    int k = 0;
    for (; k < c.n && k < max_stages; k++) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c.ev[k], c.ev[k + 1]);
        ms_out[k] = ms;
    }
    return k;
}

const char* lidargs_profile_stage_name(int stage) {
    if (!g_prof.calls || g_prof.ncalls == 0) return nullptr;
    Profiler::Call& c = g_prof.calls[(g_prof.ncalls - 1) % Profiler::MAX_CALLS];
    if (stage < 0 || stage >= c.n) return nullptr;
    return c.names[stage];
}

// Aggregate over every call recorded since lidargs_profile_enable(1): per distinct stage name the
// summed milliseconds and the number of samples.  names_out receives pointers to static strings.
int lidargs_profile_summary(const char** names_out, float* total_ms_out, int* count_out, int max_stages) {
    if (!g_prof.calls) return 0;
    int nnames = 0;
    const int ncalls = g_prof.ncalls < Profiler::MAX_CALLS ? g_prof.ncalls : Profiler::MAX_CALLS;
    for (int ci = 0; ci < ncalls; ci++) {
        Profiler::Call& c = g_prof.calls[ci];
        if (c.n == 0) continue;
        (void)hipEventSynchronize(c.ev[c.n]);
        for (int k = 0; k < c.n; k++) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c.ev[k], c.ev[k + 1]) != hipSuccess) continue;
            int j = 0;
            for (; j < nnames; j++) if (strcmp(names_out[j], c.names[k]) == 0) break;
            if (j == nnames) {
                if (nnames >= max_stages) continue;
                names_out[j] = c.names[k]; total_ms_out[j] = 0.f; count_out[j] = 0; nnames++;
            }
            total_ms_out[j] += ms; count_out[j]++;
        }
    }
    return nnames;
}

#ifdef LG_LANE_STATS
int lidargs_debug_lane_stats(unsigned long long* out, int reset) { lg::lane_stats_read(out, reset); return 16; }
#endif

void lidargs_counters_enable(int on) { g_counters_on = on ? 1 : 0; }

int lidargs_last_counters(long long* out, int n) {
    if (t_cnt.pending) {
        t_cnt.pending = false;
        if (hipEventSynchronize(t_cnt.done) == hipSuccess) {
            const unsigned long long* h = t_cnt.host;
            g_counters[1] = (long long)h[0]; g_counters[3] = (long long)h[1];
            if (h[5] & 1u) g_counters[6] = (long long)h[2];
            if (h[5] & 2u) g_counters[8] = (long long)h[3];
            if (h[5] & 4u) g_counters[9] = (long long)h[4];
        }
    }
    int k = 0;
    for (; k < n && k < 10; k++) out[k] = g_counters[k];
    return k;
}

}  // extern "C"
