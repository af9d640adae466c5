// switches.h -- every LIDARGS_* environment switch of liblidargs_hip.so, and the only file of csrc/ that reads the environment.  Host-only, no HIP
// header (tests/switches_probe.cpp is a plain C++ program around it).  A switch read once per process is a field of Switches, its initializer the
// parse rule; one read at every call is a function below the struct.  The comment on either is the switch's documentation (README's table names the same).
#pragma once
#include <stdlib.h>
#include <string.h>
#include <stddef.h>

namespace lg {
constexpr int SORT_MAX_RADIX_BITS = 11;          // the range sort of the P Gaussians: 31 key bits in 3 passes (11 + 10 + 10)
constexpr size_t SMALL_SORT_MAX = 16384;         // pairs the one-launch sort takes at most (binning.hip k_radix_sort_small: 16 rounds per wave)
// ... and up to where it is used: one CU ranks ~0.5 pairs per ns (16 waves x ~100 instructions per 64 pairs and phase on four SIMDs:
// issue-bound, tools/micro/small_sort_bench.cpp), so at 14 k pairs a pass takes 25-30 us against ~15 us for the three launches of the
// general form; below ~4 k pairs the single launch wins (4000 pairs: 12 us per pass)
constexpr size_t SMALL_SORT_DEFAULT = 4096;
inline int env_int(const char* name, int value_when_unset) { const char* e = getenv(name); return e ? atoi(e) : value_when_unset; }
inline bool env_on(const char* name) { return env_int(name, 0) != 0; }          // set and atoi != 0 ("" and "yes" are off)
inline bool env_not_off(const char* name) { return env_int(name, 1) != 0; }     // unset or atoi != 0
inline bool env_starts_with(const char* name, char c) { const char* e = getenv(name); return e && e[0] == c; }
inline int clamped(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// "3,9" -> {3, 9}: keeps the values greater than the last one kept (starting from 0) and below 255, eight at the most.  -> how many, -1 = unset
inline int parse_rounds(const char* e, int (&rounds)[8]) {
    if (!e) return -1;
    int n = 0, prev = 0;
    while (*e && n < 8) {
        const int v = atoi(e);
        if (v > prev && v < 255) { rounds[n++] = v; prev = v; }
        while (*e && *e != ',') e++;
        if (*e == ',') e++;
    }
    return n;
}

struct Switches {
    // LIDARGS_TILE_ROWS = 4, 8, 16 or 32 forces the list-tile height in pixel rows; 0 (unset, anything else) = chosen per frame (api.hip choose_tile_rows)
    int tile_rows = [] { const int v = env_int("LIDARGS_TILE_ROWS", 0); return (v == 4 || v == 8 || v == 16 || v == 32) ? v : 0; }();
    // LIDARGS_SEG_LEN, LIDARGS_MAX_SEGMENTS, LIDARGS_ROUNDS="3,9" override the segment plan (api.hip plan_segments): target entries per list
    // segment (at least 64), segment slots per list (1 .. 63, made odd), depth in segments of the gated pass-1 rounds (parse_rounds).  Unset
    // (0, 0, n_rounds -1) = the plan's own; a list that keeps no value ("", "0") is NO gated round, which is not the same as unset.
    int seg_len = getenv("LIDARGS_SEG_LEN") ? clamped(env_int("LIDARGS_SEG_LEN", 0), 64, 0x7FFFFFFF) : 0;
    int max_segments = getenv("LIDARGS_MAX_SEGMENTS") ? clamped(env_int("LIDARGS_MAX_SEGMENTS", 0), 1, 63) | 1 : 0;
    int rounds[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int n_rounds = parse_rounds(getenv("LIDARGS_ROUNDS"), rounds);
    // LIDARGS_HEAD = 0 / 1 (non-zero is 1): round 1 of the blend as the complete walk of the list heads; LIDARGS_FUSED = 0 / 1: the forward blend
    // as one launch (render.hip k_render_fused) or as the segmented launches.  -1 (unset, negative) = the plan's own; never applied to surfel plans
    int head = env_int("LIDARGS_HEAD", -1), fused = env_int("LIDARGS_FUSED", -1);
    // LIDARGS_RANGE_SORT_BITS = 8 (unset, out of range: 4 passes) .. SORT_MAX_RADIX_BITS (3 passes): digit width of an enqueue-only forward's range sort of all 31 key bits
    int range_sort_bits = [] { const int v = env_int("LIDARGS_RANGE_SORT_BITS", 8); return (v >= 8 && v <= SORT_MAX_RADIX_BITS) ? v : 8; }();
    // LIDARGS_NO_PRUNE=1 switches the conservative footprint pruning of the preprocess off (every tile / row of the reference rect is binned):
    // a diagnostic and a test instrument -- pruned entries are exactly those no pixel can take, so the results must not change
    bool no_prune = env_on("LIDARGS_NO_PRUNE");
    bool tile_key32 = env_on("LIDARGS_TILE_KEY32");                    // =1: 32-bit tile keys in the 3-D rasterizer's lists even when the tile ids fit 16 bits (A/B)
    // LIDARGS_NO_SMALL_SORT=1: never the one-launch sort; LIDARGS_SMALL_SORT_MAX = pairs up to which it is used, clamped to [0, SMALL_SORT_MAX]; unset = SMALL_SORT_DEFAULT
    bool no_small_sort = env_on("LIDARGS_NO_SMALL_SORT");
    size_t small_sort_max = [] { const char* e = getenv("LIDARGS_SMALL_SORT_MAX"); const long v = e ? atol(e) : (long)SMALL_SORT_DEFAULT;
                                 return (size_t)(v < 0 ? 0 : (v > (long)SMALL_SORT_MAX ? (long)SMALL_SORT_MAX : v)); }();
    bool range_sort_full = env_on("LIDARGS_RANGE_SORT_FULL");          // =1: the 3-D rasterizer's range sort over all 31 key bits, not the frame's key span (A/B)
    bool ng_per_lane_decode = env_on("LIDARGS_NG_PER_LANE_DECODE");    // =1: the one-anchor-per-lane decode forward, which a model without W2T gets in any case
    bool chamfer_brute = env_on("LIDARGS_CHAMFER_BRUTE");              // =1: the brute-force chamfer kernel only, no grid search in front (A/B, tests: the round-3 path)
    bool work_lists = env_not_off("LIDARGS_WORK_LISTS");               // =0: the backward blend over the (patch, segment) slot grid, not the work list (A/B, tests)
    bool range_sort_buckets = env_not_off("LIDARGS_RANGE_SORT_BUCKETS");   // =0: the LSD passes instead of the bucketed range sort (A/B, tests)
    bool range_sort_packed = env_not_off("LIDARGS_RANGE_SORT_PACKED");     // =0: the bucketed sort gathers its 4-byte span records behind it, round 5's form (A/B)
    // LIDARGS_WALK2 (bits; unset = 7): 1 = the second form of the T-only walk (the surfel pass 1 reads this bit too), 2 = of the full walk, 4 = of the backward walk; 0 = the first forms (A/B)
    int walk2 = env_int("LIDARGS_WALK2", 7);
    int fused_waves = [] { const int v = env_int("LIDARGS_FUSED_WAVES", 8); return (v == 4 || v == 16) ? v : 8; }();   // waves per workgroup of the fused forward blend: 4 or 16, else 8
    int p2_group = clamped(env_int("LIDARGS_P2_GROUP", 0), 0, 64);     // segments a pass-2 workgroup walks in a row; 0 (unset) = by segment length (render.hip pass2_group)
    int sort_items = env_int("LIDARGS_SORT_ITEMS", 0);                 // 8: half-size radix blocks wherever they fit; other non-zero (16): full blocks; 0 (unset): by size
};
inline Switches read_switches() { return Switches(); }                 // a pure function of the environment
inline const Switches& switches() { static const Switches s = read_switches(); return s; }   // the library's one copy, read at the first call
// n pairs sort in the single launch of one workgroup: asked by the sort, by the prediction of the side it ends on and by the bucketed range sort's lower limit (binning.hip)
inline bool uses_small_sort(size_t n) { return n <= switches().small_sort_max && !switches().no_small_sort; }
// ---- read at every call ----
// LIDARGS_DETERMINISTIC=1: a supported mode, not a diagnostic -- lidargs_forward makes buffers on which every lidargs_backward is a pure
// function of its inputs (lidargs_common.h "deterministic accumulation").  Read at EVERY call (a caller may flip it between two frames of
// one process), and by forward entry points only: a backward takes the mode from the buffers.  Unset, empty, 0: off.
inline bool deterministic_requested() { return env_on("LIDARGS_DETERMINISTIC"); }
// LIDARGS_DEPTH: which depth lidargs_forward returns.  Read at EVERY call, by forward entry points only (the mode travels in the buffers,
// like the deterministic one).  Only the literal names of the table below select a mode: unset, empty, anything else = Expected.
enum class DepthMode {
    // the expected range, sum of range x alpha x T: the default
    Expected,
    // LIDARGS_DEPTH=median: a supported mode -- lidargs_forward returns the median range per pixel (the range of the Gaussian at which the
    // transmittance falls through one half: render.hip k_render_median) instead of the expected range, and makes buffers on which every
    // lidargs_backward sends a pixel's depth gradient to that one Gaussian ("median buffers").
    Median,
    // LIDARGS_DEPTH=strongest: the other supported value of the same switch -- the range of the pixel's strongest return, the entry with the
    // largest blend weight alpha x T (render.hip k_render_strongest).  Its buffers are median buffers to every backward: the depth is one
    // Gaussian's, named in the same id plane.
    Strongest,
    // LIDARGS_DEPTH=second: the third supported value -- the range of the pixel's SECOND return, what a LiDAR in multi-return mode reports
    // behind its strongest one (render.hip k_render_second).  THE RULE, stated here and in DESIGN 4d; everything else cites it.  Per pixel,
    // over its list in blend order, entries are taken and count exactly as under `strongest` (power <= 0, alpha = min(0.99, o exp(power))
    // >= 1/255; the entry at which T (1 - alpha) < 1e-4 ends the pixel and does not count), with the weight w = alpha T:
    //   1. s = the strongest return, picked bit for bit by the strongest rule: the largest w, the nearer entry among equal weights;
    //   2. the candidates are the counting entries j != s with |depths[j] - depths[s]| >= G, compared in float32 on the float32 ranges the
    //      records hold (a sensor cannot separate echoes closer than its pulse length; G = return_gap() below);
    //   3. the second return is the candidate with the largest w, the nearer one among equal weights: its range, its id in the id plane;
    //   4. no candidate (no taker, a single taker, every other taker inside the gap): range 0, id 0xFFFFFFFF, as a pixel without a taker.
    // With G = 0 this is the second-largest weight.  Its buffers are median buffers, like `strongest`'s.
    Second
};
// The values' names, by value: the only place of csrc/ that spells them (diff_lidargs_rasterization.depth_mode() is the same table in
// Python), and the picked ones as the error messages list them.
constexpr int DEPTH_MODE_COUNT = (int)DepthMode::Second + 1;             // what every table indexed by a DepthMode is checked against
constexpr const char* DEPTH_MODE_NAMES[] = {"expected", "median", "strongest", "second"};
static_assert(sizeof(DEPTH_MODE_NAMES) / sizeof(DEPTH_MODE_NAMES[0]) == DEPTH_MODE_COUNT, "one name per DepthMode");
#define LG_PICKED_DEPTH_NAMES "median, strongest, second"
constexpr bool lists_the_picked_names(const char* list) {
    for (int i = 1; i < DEPTH_MODE_COUNT; i++) {
        for (const char* n = DEPTH_MODE_NAMES[i]; *n;) if (*list++ != *n++) return false;
        if (i < DEPTH_MODE_COUNT - 1 && (*list++ != ',' || *list++ != ' ')) return false;
    }
    return *list == 0;
}
static_assert(lists_the_picked_names(LG_PICKED_DEPTH_NAMES), "LG_PICKED_DEPTH_NAMES is every name but the first, joined by \", \"");
inline DepthMode depth_mode() {
    const char* e = getenv("LIDARGS_DEPTH");
    for (int i = 1; e && i < DEPTH_MODE_COUNT; i++) if (strcmp(e, DEPTH_MODE_NAMES[i]) == 0) return (DepthMode)i;
    return DepthMode::Expected;
}
// any of them but Expected: the depth of a forward is one Gaussian's range, not the expected range (what the other entry points refuse)
inline bool picked(DepthMode m) { return m != DepthMode::Expected; }
// LIDARGS_RETURN_GAP = G of the rule above in metres, as a float32.  Read at every forward, by lidargs_forward only, and used only under
// LIDARGS_DEPTH=second; it does not travel in the buffers (a backward does not know the rule).  Accepted if and only if the WHOLE string
// matches [0-9]+(\.[0-9]*)?|\.[0-9]+ -- no sign, exponent or blank -- and its value, rounded to double and then to float32, is finite;
// unset, empty or anything else: 0.  (diff_lidargs_rasterization.return_gap() is the same rule in Python.)
inline float return_gap() {
    const char* e = getenv("LIDARGS_RETURN_GAP");
    if (!e) return 0.f;
    const char* p = e;
    size_t whole = 0, frac = 0;
    while (*p >= '0' && *p <= '9') { p++; whole++; }
    const bool dot = *p == '.';
    if (dot) { p++; while (*p >= '0' && *p <= '9') { p++; frac++; } }
    if (*p != 0 || (whole == 0 && !(dot && frac > 0))) return 0.f;
    char* end = nullptr;
    const double v = strtod(e, &end);
    if (end != p || !(v < 0x1.ffffffp127)) return 0.f;    // (2^128 - 2^103: from there on the nearest float32 is infinity)
    return (float)v;
}
// LIDARGS_NG_FORWARD_T16=0, LIDARGS_NG_BACKWARD_T16=0 (first character '0'): the decode's forward / backward on the 32x32x2 kernels, which
// k = 8, 10 take in any case, instead of the 16x16x4 ones (A/B, test variants)
inline bool ng_forward_t16_allowed() { return !env_starts_with("LIDARGS_NG_FORWARD_T16", '0'); }
inline bool ng_backward_t16_allowed() { return !env_starts_with("LIDARGS_NG_BACKWARD_T16", '0'); }
// LIDARGS_NG_T16_PASSES=1 (first character '1'): the four MLPs of the 16x16x4 decode backward in one launch (A/B); default two launches
inline bool ng_t16_two_pass() { return !env_starts_with("LIDARGS_NG_T16_PASSES", '1'); }
inline int ng_t16_stagger() { return env_int("LIDARGS_NG_T16_STAGGER", 0); }   // wave w of k_ng_backward_t16 waits w x this x 8 k clocks before its first tile (experiments); unset = 0
// LIDARGS_RANGE_SORT_BUCKET_BITS = one of the bucketed range sort's two widths (binning.hip BUCKET_BITS, BUCKET_BITS_BIG) forces that form at any
// size; 0 (unset, anything else) = by size.  For tests: the CPU checker cannot run frames above 4 M Gaussians; the suite switches it in one process.
inline int forced_bucket_bits(int bits, int bits_big) { const int v = env_int("LIDARGS_RANGE_SORT_BUCKET_BITS", 0); return (v == bits || v == bits_big) ? v : 0; }
}  // namespace lg
