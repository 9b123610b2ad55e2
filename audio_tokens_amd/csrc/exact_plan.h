// exact_plan.h -- the decisions of at_assign_pruned_f32 (exact_search.cpp) that need no device: which route a call
// takes, how its redo is sized, and what its statistics words add to the context's totals.  Pure host functions, no
// HIP header: tests/host_harness/exact_plan_host.cpp compiles them with g++ (tests/test_exact_plan_host.py).
#pragma once
#include <cstddef>
#include <cstdint>

// the rows a filter sweep lists for the redo: 64 sub-lists (counters at misc[64 ..] of its 128 statistics words)
constexpr unsigned AT_AMB_SUBLISTS = 64;

namespace exact_plan {

// where the distances of a call come from
enum DistPass {
    DIST_FROM_SWEEP = 0,   // no pass of their own: the sweep writes them (exact fp32 sweep, or a guess generator's approximate ones)
    DIST_FROM_TODO,        // at_exact_dist_todo: the fused sweep wrote the guess distances, the rows that moved get theirs
    DIST_FROM_ROWS,        // at_exact_dist_rows: from the pre-pass distances of the guesses
    DIST_FROM_FINISH       // at_filter_finish: rides in the launch that redoes the listed rows
};

struct Plan {
    bool image_up_front;    // the fp32 image is built before the sweep (no filter); else only for a long-list redo
    bool prepass_separate;  // the pre-pass runs as a kernel of its own
    bool prepass_fused;     // ... or in the prologue of the filter sweep
    bool filter;            // stage 1 is the fp16-split filter: its workspace is claimed, a statistics slot is used
    bool stage2;            // the filter's listed rows are redone (exact calls only)
    bool async_form;        // the redo reads the list length on the device, the statistics go to a ring slot
    bool sweep_dist;        // the filter sweep is handed the caller's dist
    DistPass dist;
};

// The route of a call, from its arguments (guess_only, use_filter, prepass_done, dist asked for), the switches
// filter_fused / filter_sync and the context's force_sync.
inline Plan plan(bool guess_only, bool use_filter, bool prepass_done, bool want_dist, int filter_fused, int filter_sync,
                 int force_sync) {
    Plan p{};
    p.filter = use_filter;
    p.image_up_front = !use_filter;
    // exact filtered calls without a pre-pass done by the caller: the sweep does it in its prologue
    p.prepass_fused = use_filter && !guess_only && !prepass_done && filter_fused != 0;   // (switch: 0 = separate pre-pass kernel)
    p.prepass_separate = !prepass_done && !p.prepass_fused;
    p.stage2 = use_filter && !guess_only;
    p.async_form = p.stage2 && !force_sync && filter_sync != 1;
    p.sweep_dist = use_filter && want_dist && (p.prepass_fused || guess_only);
    p.dist = DIST_FROM_SWEEP;
    if (use_filter && want_dist && !guess_only)
        p.dist = !p.prepass_fused ? DIST_FROM_ROWS : p.async_form ? DIST_FROM_FINISH : DIST_FROM_TODO;
    return p;
}

// Asynchronous form: workgroups of the redo, enough for a list of 1.5 % of the rows in one go (they stride over any length).
inline int64_t async_redo_wgs(int64_t n) {
    const int64_t wgs = n / 64;
    return wgs < 256 ? 256 : wgs > 65535 ? 65535 : wgs;
}

// Synchronous form: what a list of `listed` of n rows gets.  Short lists: one workgroup per row on the vector ALU;
// long ones (badly conditioned data, centroids outside the fp16 range): the fp32 MFMA sweep over the listed rows,
// padded to at least 64 of them.
enum RedoKind { REDO_NONE = 0, REDO_SHORT, REDO_LONG };
struct SyncRedo {
    RedoKind kind;
    int64_t count;   // REDO_SHORT: workgroups; REDO_LONG: rows of the fp32 sweep
};
inline bool long_list(int64_t listed, int64_t rows) { return listed * 16 > rows; }
inline SyncRedo sync_redo(int64_t listed, int64_t n) {
    if (listed == 0) return {REDO_NONE, 0};
    if (!long_list(listed, n)) return {REDO_SHORT, listed < 65535 ? listed : 65535};
    return {REDO_LONG, listed < 64 ? 64 : listed};
}

// The context's running totals (at_filter_stats) and the verdict the next call's plan reads.
struct Totals {
    int64_t rows, listed;      // rows swept / rows handed to the redo
    int64_t tiles, refined;    // 32x32 tiles multiplied (hi*hi) / refined (lo products too)
    int force_sync;            // a call listed more than rows/16: exact calls take the synchronous form
};

// One call's 128 statistics words folded into the totals; returns the length of its list.
inline int64_t fold(Totals& t, const unsigned* words, int64_t rows) {
    int64_t listed = 0;
    for (unsigned s = 0; s < AT_AMB_SUBLISTS; s++) listed += words[64 + s];
    t.rows += rows;
    t.listed += listed;
    t.tiles += words[4];
    t.refined += words[5];
    return listed;
}
// ... of an asynchronous call, when its ring slot is read: a long list switches the context to the synchronous form
inline void fold_ring_slot(Totals& t, const unsigned* words, int64_t rows) {
    if (long_list(fold(t, words, rows), rows)) t.force_sync = 1;
}
// ... of a synchronous call, at once: a short list switches back (the data behave again)
inline int64_t fold_sync_call(Totals& t, const unsigned* words, int64_t rows) {
    const int64_t listed = fold(t, words, rows);
    if (!long_list(listed, rows)) t.force_sync = 0;
    return listed;
}

// ---- the shape of the filter sweep and the order its row blocks start in ------------------------------------------
// Rows per wave = 32 * tiles.  Lloyd-sized exact sweeps (rows sorted by guess, <= 8 M of them) run two tiles per wave
// at three waves per SIMD; short ones (a shard of an N-GPU run) one tile at four waves; the long tokenise sweeps, the
// guess generators and every sweep with a pre-pass of its own keep four tiles at two waves (d = 128: two tiles, its
// fragment sets leave no registers for four).  filter_nb = 1 | 2 | 4 forces the choice, filter_wps2 the two-wave forms.
constexpr int64_t ONE_TILE_MAX_ROWS = (int64_t)1 << 19;
constexpr int64_t TWO_TILE_MAX_ROWS = (int64_t)8 << 20;
struct SweepShape {
    int tiles;   // 32-row tiles per wave (1, 2, 4)
    int wps;     // waves per SIMD the kernel is built for
};
inline SweepShape sweep_shape(bool fused, int d, int64_t n, int filter_nb, int filter_wps2) {
    if (d == 128) return {2, 2};
    const bool one_tile = fused && !filter_wps2 && (filter_nb ? filter_nb == 1 : n <= ONE_TILE_MAX_ROWS);
    if (one_tile) return {1, 4};
    const bool wps3 = fused && (filter_nb ? filter_nb == 2 : n <= TWO_TILE_MAX_ROWS) && !filter_wps2;
    if (wps3) return {2, 3};
    return {filter_nb == 2 ? 2 : 4, 2};
}

// Block schedules (prune.hip makes them beside the visiting order, the filter sweep starts its row blocks in their
// order: widest need sets first, so that no long block starts on an emptying chip).  A weight per 32-row tile in
// 0..255 -> a class per block of 1, 2 or 4 tiles (the largest of its tiles' weights, its top CLASS_BITS bits) -> blocks
// in descending class, ascending index within a class.
constexpr int SCHED_WEIGHT_MAX = 255;
constexpr int SCHED_CLASS_BITS = 4;
constexpr int SCHED_CLASSES = 1 << SCHED_CLASS_BITS;
constexpr int SCHED_CHUNK = 2048;   // blocks per workgroup of the counting sort
constexpr int sched_class(int weight) { return weight >> (8 - SCHED_CLASS_BITS); }
inline int sched_table_index(int tiles) { return tiles == 1 ? 0 : tiles == 2 ? 1 : tiles == 4 ? 2 : -1; }

// One half of the double buffer: the tile weights, the histograms of the counting sort, and the three tables.
struct SchedLayout {
    int64_t tiles;          // 32-row tiles of n rows
    int64_t blocks[3];      // row blocks of 1, 2, 4 tiles
    int64_t chunks;         // workgroups of the counting sort of the one-tile table (the others use the first of them)
    size_t weight_off, hist_off, table_off[3];   // bytes from the start of the half
    size_t bytes;           // of one half, a multiple of 256
};
inline SchedLayout sched_layout(int64_t n) {
    SchedLayout l{};
    l.tiles = (n + 31) / 32;
    for (int t = 0; t < 3; t++) l.blocks[t] = (l.tiles + (1 << t) - 1) >> t;
    l.chunks = (l.tiles + SCHED_CHUNK - 1) / SCHED_CHUNK;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t off = at; at = (at + bytes + 255) & ~(size_t)255; return off; };
    l.weight_off = take((size_t)l.tiles);
    l.hist_off = take(sizeof(uint32_t) * 3 * (size_t)l.chunks * SCHED_CLASSES);
    for (int t = 0; t < 3; t++) l.table_off[t] = take(sizeof(uint32_t) * (size_t)l.blocks[t]);
    l.bytes = at;
    return l;
}

// Where a sweep takes its block order from.  A table made beside a visiting order is used only by a sweep over that
// very order buffer with the same n (any order of n rows is served correctly by any permutation of its blocks, so a
// stale table behind a reused buffer costs speed at most; a table of another n would name blocks that do not exist
// or miss some).  A schedule installed through the debug hook goes first, for sweeps of exactly its block count.
enum SchedPath { SCHED_IDENTITY = 0, SCHED_TABLE0, SCHED_TABLE1, SCHED_INSTALLED };
struct SchedTag {
    const void* order;   // the order_out the table was built beside
    int64_t n;
    int valid;
};
inline SchedPath sched_path(int block_sched, bool exact_sweep, const void* order, int64_t n, int tiles, int64_t blocks,
                            const SchedTag& t0, const SchedTag& t1, int64_t installed_blocks) {
    if (!exact_sweep || sched_table_index(tiles) < 0) return SCHED_IDENTITY;
    if (installed_blocks > 0 && installed_blocks == blocks) return SCHED_INSTALLED;
    if (!block_sched || !order) return SCHED_IDENTITY;
    if (t0.valid && t0.order == order && t0.n == n) return SCHED_TABLE0;
    if (t1.valid && t1.order == order && t1.n == n) return SCHED_TABLE1;
    return SCHED_IDENTITY;
}

}  // namespace exact_plan
