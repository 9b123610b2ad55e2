// exact_plan.h -- the decisions of at_assign_pruned_f32 (exact_search.cpp) that need no device: which route a call
// takes, how its redo is sized, and what its statistics words add to the context's totals.  Pure host functions, no
// HIP header: tests/host_harness/exact_plan_host.cpp compiles them with g++ (tests/test_exact_plan_host.py).
#pragma once
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

}  // namespace exact_plan
