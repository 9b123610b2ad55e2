// The host-only decisions of the exact pruned search (audio_tokens_amd/csrc/exact_plan.h) behind a C interface:
// the route of a call, the sizing of its redo and the fold of its statistics words (tests/test_exact_plan_host.py).
#include "../../audio_tokens_amd/csrc/exact_plan.h"

extern "C" {

// out: image_up_front, prepass_separate, prepass_fused, filter, stage2, async_form, sweep_dist, dist (exact_plan::DistPass)
void exact_plan_host_plan(int guess_only, int use_filter, int prepass_done, int want_dist, int filter_fused, int filter_sync,
                          int force_sync, int* out) {
    const exact_plan::Plan p = exact_plan::plan(guess_only != 0, use_filter != 0, prepass_done != 0, want_dist != 0, filter_fused,
                                                filter_sync, force_sync);
    out[0] = p.image_up_front; out[1] = p.prepass_separate; out[2] = p.prepass_fused; out[3] = p.filter;
    out[4] = p.stage2; out[5] = p.async_form; out[6] = p.sweep_dist; out[7] = (int)p.dist;
}

int64_t exact_plan_host_async_redo_wgs(int64_t n) { return exact_plan::async_redo_wgs(n); }

// out: kind (0 nothing, 1 short, 2 long), count
void exact_plan_host_sync_redo(int64_t listed, int64_t n, int64_t* out) {
    const exact_plan::SyncRedo r = exact_plan::sync_redo(listed, n);
    out[0] = (int64_t)r.kind;
    out[1] = r.count;
}

// totals (in / out): rows, listed, tiles, refined, force_sync.  ring != 0: as at_filter_resolve_pending folds a slot;
// else as the synchronous form folds its own words.  Returns the list length the synchronous form goes on with (-1: ring).
int64_t exact_plan_host_fold(int ring, const unsigned* words, int64_t rows, int64_t* totals) {
    exact_plan::Totals t{totals[0], totals[1], totals[2], totals[3], (int)totals[4]};
    int64_t listed = -1;
    if (ring) exact_plan::fold_ring_slot(t, words, rows);
    else listed = exact_plan::fold_sync_call(t, words, rows);
    totals[0] = t.rows; totals[1] = t.listed; totals[2] = t.tiles; totals[3] = t.refined; totals[4] = t.force_sync;
    return listed;
}

}
