// What lidar-gs_amd/csrc/switches.h reads from this process' environment, one `LIDARGS_NAME=value` line per switch
// (tests/test_switches_cpu.py).  No GPU, no HIP: g++ -std=c++17 -I lidar-gs_amd/csrc tests/switches_probe.cpp
#include "switches.h"
#include <stdio.h>

int main() {
    const lg::Switches s = lg::read_switches();
    printf("LIDARGS_TILE_ROWS=%d\nLIDARGS_SEG_LEN=%d\nLIDARGS_MAX_SEGMENTS=%d\n", s.tile_rows, s.seg_len, s.max_segments);
    printf("LIDARGS_ROUNDS=");
    if (s.n_rounds < 0) printf("unset");
    for (int k = 0; k < s.n_rounds; k++) printf(k ? ",%d" : "%d", s.rounds[k]);
    printf("\nLIDARGS_HEAD=%d\nLIDARGS_FUSED=%d\nLIDARGS_RANGE_SORT_BITS=%d\n", s.head, s.fused, s.range_sort_bits);
    printf("LIDARGS_NO_PRUNE=%d\nLIDARGS_TILE_KEY32=%d\nLIDARGS_NO_SMALL_SORT=%d\nLIDARGS_SMALL_SORT_MAX=%zu\n", s.no_prune, s.tile_key32, s.no_small_sort, s.small_sort_max);
    printf("LIDARGS_RANGE_SORT_FULL=%d\nLIDARGS_NG_PER_LANE_DECODE=%d\nLIDARGS_CHAMFER_BRUTE=%d\n", s.range_sort_full, s.ng_per_lane_decode, s.chamfer_brute);
    printf("LIDARGS_WORK_LISTS=%d\nLIDARGS_RANGE_SORT_BUCKETS=%d\nLIDARGS_RANGE_SORT_PACKED=%d\n", s.work_lists, s.range_sort_buckets, s.range_sort_packed);
    printf("LIDARGS_WALK2=%d\nLIDARGS_FUSED_WAVES=%d\nLIDARGS_P2_GROUP=%d\nLIDARGS_SORT_ITEMS=%d\n", s.walk2, s.fused_waves, s.p2_group, s.sort_items);
    printf("LIDARGS_DETERMINISTIC=%d\nLIDARGS_NG_FORWARD_T16=%d\nLIDARGS_NG_BACKWARD_T16=%d\n", lg::deterministic_requested(), lg::ng_forward_t16_allowed(), lg::ng_backward_t16_allowed());
    printf("LIDARGS_NG_T16_PASSES=%d\nLIDARGS_NG_T16_STAGGER=%d\n", lg::ng_t16_two_pass() ? 2 : 1, lg::ng_t16_stagger());
    printf("LIDARGS_RANGE_SORT_BUCKET_BITS=%d\n", lg::forced_bucket_bits(10, 11));   // any two widths: binning.hip hands in its own
    return 0;
}
