// Host harness of tests/test_block_schedule_host.py: the block-schedule decisions of csrc/exact_plan.h behind a C
// interface (g++ only, no HIP).
#include "../../audio_tokens_amd/csrc/exact_plan.h"

extern "C" {

// out = {tiles per wave, waves per SIMD}
void block_schedule_host_shape(int fused, int d, int64_t n, int filter_nb, int filter_wps2, int* out) {
    const exact_plan::SweepShape s = exact_plan::sweep_shape(fused != 0, d, n, filter_nb, filter_wps2);
    out[0] = s.tiles;
    out[1] = s.wps;
}

void block_schedule_host_limits(int64_t* out) {
    out[0] = exact_plan::ONE_TILE_MAX_ROWS;
    out[1] = exact_plan::TWO_TILE_MAX_ROWS;
}

// tags: {order, n, valid} twice, orders as integers
int block_schedule_host_path(int block_sched, int exact_sweep, int64_t order, int64_t n, int tiles, int64_t blocks,
                             const int64_t* tags, int64_t installed_blocks) {
    const exact_plan::SchedTag t0{reinterpret_cast<const void*>(tags[0]), tags[1], (int)tags[2]};
    const exact_plan::SchedTag t1{reinterpret_cast<const void*>(tags[3]), tags[4], (int)tags[5]};
    return (int)exact_plan::sched_path(block_sched, exact_sweep != 0, reinterpret_cast<const void*>(order), n, tiles, blocks, t0, t1,
                                       installed_blocks);
}

// out = {tiles, blocks[3], chunks, weight_off, hist_off, table_off[3], bytes}
void block_schedule_host_layout(int64_t n, int64_t* out) {
    const exact_plan::SchedLayout l = exact_plan::sched_layout(n);
    out[0] = l.tiles;
    for (int t = 0; t < 3; t++) out[1 + t] = l.blocks[t];
    out[4] = l.chunks;
    out[5] = (int64_t)l.weight_off;
    out[6] = (int64_t)l.hist_off;
    for (int t = 0; t < 3; t++) out[7 + t] = (int64_t)l.table_off[t];
    out[10] = (int64_t)l.bytes;
}

int block_schedule_host_class(int weight) { return exact_plan::sched_class(weight); }
int block_schedule_host_constants(int which) {
    return which == 0 ? exact_plan::SCHED_WEIGHT_MAX : which == 1 ? exact_plan::SCHED_CLASSES : exact_plan::SCHED_CHUNK;
}

}  // extern "C"
