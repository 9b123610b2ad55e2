// exact_search.cpp -- the host side of the exact pruned nearest-centroid search: at_assign_pruned_f32, its pre-pass and
// probe entry points, the statistics ring of its asynchronous form and at_filter_stats.  No kernel lives here: the
// launches are at_prune_prepass (prune.hip), at_filter_* / at_exact_dist_* / at_amb_compact (filter.hip) and
// at_pruned_image_* / at_pruned_sweep_f32 (assign.hip); the decisions that need no device are in exact_plan.h.
//
// A filtered exact call finishes in one of four ways (tests/test_gpu_hard_data.py walks all of them):
//   asynchronous form  the redo kernels read the list length on the device, whatever it is (finish_async); the call's
//                      statistics words go to a ring slot and are folded into the totals at a later call or query.  A
//                      call that turns out to have listed more than n/16 rows (badly scaled data) was still answered
//                      correctly, but switches the context to the synchronous form;
//   synchronous form   the words are read at once: nothing listed, a short list (at_filter_redo_rows), or a long one
//                      (finish_sync_long: the fp32 MFMA sweep over the listed rows).  A short list switches back.
#include "at_internal.h"

namespace {

// Sizes every entry point over grouped centroids shares (n_min: 20 where the fp32 sweep may run, 1 for the guess generator).
bool grouped_sizes_ok(int64_t n, int64_t n_min, int d, int k, int ng) {
    return (d == 64 || d == 128) && n >= n_min && n < (int64_t)UINT32_MAX && ng > 0 && ng <= 512 && ng * 32 >= k;
}

// ---- workspace -------------------------------------------------------------------------------------------------
// The pre-pass outputs, for max(n, 64) rows: the long-list redo runs the pre-pass and the sweep over at least 64 rows,
// whatever n is.  Nothing of the filter is touched.
int claim_prepass(at_ctx* ctx, at_exact_call& call) {
    const int64_t n_ws = call.n < 64 ? 64 : call.n;
    call.ngw = (call.ng + 31) / 32;
    call.bd = static_cast<float*>(at_ws(ctx, WS_PRUNE_BD, sizeof(float) * (size_t)n_ws, call.stream));
    call.mask = static_cast<uint32_t*>(
        at_ws(ctx, WS_PRUNE_MASK, sizeof(uint32_t) * (size_t)((n_ws + 31) / 32) * call.ngw, call.stream));
    return call.bd && call.mask ? AT_OK : AT_E_NOMEM;
}

// The filter's statistics words and its five arrays of 64 sub-lists: list | sorted | order | hints | aux.
int claim_filter(at_ctx* ctx, at_exact_call& call) {
    call.lstride = at_amb_stride(call.n);
    call.amb_cap = at_amb_cap(call.n);
    call.misc = static_cast<unsigned*>(at_ws(ctx, WS_FILTER_MISC, 1024, call.stream));
    call.list = static_cast<uint32_t*>(at_ws(ctx, WS_FILTER_LIST, sizeof(uint32_t) * 5 * call.lstride, call.stream));
    if (!call.misc || !call.list) return AT_E_NOMEM;
    call.sorted = call.list + call.lstride;
    call.order_amb = call.sorted + call.lstride;
    call.hint_amb = call.order_amb + call.lstride;
    call.aux = call.hint_amb + call.lstride;
    return AT_OK;
}

// ---- the statistics ring (at_internal.h: at_filter_slot) ---------------------------------------------------------
// Life of a slot: claimed by at_filter_use_slot (timed = 0) -> the sweep records ev[0], ev[1] around its kernel only
// under the switch filter_timing and then sets timed = 1 -> the call queues the copy of its statistics words and
// records `copied` -> pushed (count++) -> at_filter_resolve_pending reads the words once `copied` has completed and the
// two timing events only if timed is set.  hipEventElapsedTime on an event that was never recorded returns
// hipErrorInvalidResourceHandle and leaves it pending in the thread: it is not called on such events, and its result
// is consumed where it is tolerated.

// The stage-1 kernel time of the call whose events `fs` lent (both were recorded before its words were read, on the
// same stream: they have completed).
void fold_timing(at_filter_state& f, at_filter_slot& fs) {
    float ms = 0.0f;
    if (fs.timed && AT_HIP_TOLERATE(hipEventElapsedTime(&ms, fs.ev[0], fs.ev[1])) == hipSuccess) {
        f.ms += ms;
        f.launches++;
    }
    fs.timed = 0;
}

// The slot of a call that is about to queue its filter sweep.  Asynchronous form: the next of the ring, waiting for the
// oldest only when the host is a whole ring ahead of the device.  Synchronous form: the spare, with every pending slot
// folded first (it reads its own words at once: keep the order).  Guess generators leave no words behind: the spare.
int take_slot(at_ctx* ctx, const exact_plan::Plan& plan, int* slot) {
    at_filter_state& f = ctx->filter;
    *slot = AT_FILTER_RING;
    if (plan.async_form) {
        if (f.count == AT_FILTER_RING) {
            AT_HIP(hipEventSynchronize(f.ring[f.head].copied));
            const int rc = at_filter_resolve_pending(ctx, false);
            if (rc) return rc;
        }
        *slot = (f.head + f.count) % AT_FILTER_RING;
    } else if (plan.stage2) {
        const int rc = at_filter_resolve_pending(ctx, true);
        if (rc) return rc;
    }
    return at_filter_use_slot(ctx, *slot);
}

// ---- the three ways to finish a filtered exact call that listed rows -----------------------------------------------
int finish_async(at_ctx* ctx, const at_exact_call& call, const exact_plan::Plan& plan, int slot) {
    at_filter_slot& fs = ctx->filter.ring[slot];
    const int64_t wgs = exact_plan::async_redo_wgs(call.n);
    const int rc = plan.dist == exact_plan::DIST_FROM_FINISH ? at_filter_finish(ctx, call, wgs) : at_filter_redo_rows(ctx, call, wgs);
    if (rc) return rc;
    AT_HIP(hipMemcpyAsync(fs.host_misc, call.misc, 128 * sizeof(unsigned), hipMemcpyDeviceToHost, call.stream));
    AT_HIP(hipEventRecord(fs.copied, call.stream));
    fs.rows = call.n;
    ctx->filter.count++;
    return AT_OK;
}

// The listed rows in one piece (listed <= n < the stride: the contiguous copy fits the `sorted` / `order_amb` arrays; it
// then moves to the front of `list`), sorted and padded to n2 rows, then a fresh pre-pass and the fp32 sweep over them.
int finish_sync_long(at_ctx* ctx, const at_exact_call& call, int64_t listed, int64_t n2) {
    int rc = at_pruned_image_build(ctx, call);
    if (rc) return rc;
    rc = at_amb_compact(ctx, call);
    if (rc) return rc;
    AT_HIP(hipMemcpyAsync(call.list, call.sorted, sizeof(uint32_t) * listed, hipMemcpyDeviceToDevice, call.stream));
    rc = at_filter_gather_ambiguous(ctx, call, listed, n2);
    if (rc) return rc;
    rc = at_prune_prepass(ctx, call, n2, call.order_amb, call.hint_amb, 0);
    if (rc) return rc;
    return at_pruned_sweep_f32(ctx, call, n2, call.order_amb, call.hint_amb);
}

// The synchronous form: the call's words at once, then the finish they ask for.
int finish_sync(at_ctx* ctx, const at_exact_call& call) {
    unsigned host_misc[128];
    AT_HIP(hipMemcpyAsync(host_misc, call.misc, sizeof host_misc, hipMemcpyDeviceToHost, call.stream));
    AT_HIP(hipStreamSynchronize(call.stream));
    const int64_t listed = exact_plan::fold_sync_call(ctx->filter.tot, host_misc, call.n);
    fold_timing(ctx->filter, ctx->filter.ring[AT_FILTER_RING]);
    const exact_plan::SyncRedo redo = exact_plan::sync_redo(listed, call.n);
    if (redo.kind == exact_plan::REDO_SHORT) return at_filter_redo_rows(ctx, call, redo.count);
    if (redo.kind == exact_plan::REDO_LONG) return finish_sync_long(ctx, call, listed, redo.count);
    return AT_OK;
}

// The driver: plan, claim, pre-pass, sweep, distance pass, finish.
int exact_search(at_ctx* ctx, at_exact_call& call, int mode, bool prepass_done, bool use_filter) {
    if (use_filter) {   // verdicts of earlier calls whose words have arrived (polled, not waited for) count for this plan
        const int rcp = at_filter_resolve_pending(ctx, false);
        if (rcp) return rcp;
    }
    const exact_plan::Plan plan = exact_plan::plan(mode != 0, use_filter, prepass_done, call.dist != nullptr, ctx->dbg.filter_fused,
                                                   ctx->dbg.filter_sync, ctx->filter.tot.force_sync);
    int rc = at_pruned_image_claim(ctx, call);
    if (rc) return rc;
    rc = claim_prepass(ctx, call);
    if (rc) return rc;
    if (plan.image_up_front) {
        rc = at_pruned_image_build(ctx, call);
        if (rc) return rc;
    }
    if (plan.prepass_separate) {
        rc = at_prune_prepass(ctx, call, call.n, call.order, call.hint_sorted, mode);
        if (rc) return rc;
    }
    if (!plan.filter) return at_pruned_sweep_f32(ctx, call, call.n, call.order, call.hint_sorted);
    // Stage 1: the fp16-split filter names the winner of every row whose runner-up is provably out of reach and lists
    // the others; stage 2 redoes the listed rows in fp32.  Guess generators need neither the list nor stage 2.
    int slot = AT_FILTER_RING;
    rc = take_slot(ctx, plan, &slot);
    if (rc) return rc;
    rc = claim_filter(ctx, call);
    if (rc) return rc;
    rc = at_filter_sweep(ctx, call, plan.stage2 ? 1 : 0, plan.prepass_fused, plan.sweep_dist ? call.dist : nullptr, nullptr);
    if (rc) return rc;
    // (guess generators wrote an approximate distance themselves: it only orders the next visit)
    if (plan.dist == exact_plan::DIST_FROM_TODO) rc = at_exact_dist_todo(ctx, call);
    if (plan.dist == exact_plan::DIST_FROM_ROWS) rc = at_exact_dist_rows(ctx, call);
    if (rc || !plan.stage2) return rc;
    return plan.async_form ? finish_async(ctx, call, plan, slot) : finish_sync(ctx, call);
}

}  // namespace

// ---- block schedules (exact_plan.h: sched_path; made in prune.hip beside the visiting order) -------------------------
// Why a sweep may start its blocks by a table: any permutation of the blocks of a launch gives the same output (each
// block records its rows by position), so a table that is stale -- made for an order that has
// since been overwritten in place, or whose buffer now holds another order of the same n -- costs speed at most.  A
// table of another row count, or one read while it is rewritten, could name a block twice and another never: hence
// the tag (order buffer, n), the two halves by call parity, their guards, and the visiting order as the fall-back.
int at_block_sched_pick(at_ctx* ctx, const at_exact_call& call, bool exact_sweep, int tiles, int64_t blocks,
                        const uint32_t** sched, int* half) {
    at_block_sched_state& s = ctx->sched;
    *sched = nullptr;
    *half = -1;
    const exact_plan::SchedPath path = exact_plan::sched_path(ctx->dbg.block_sched, exact_sweep, call.order, call.n, tiles, blocks,
                                                              s.tag[0], s.tag[1], s.installed_blocks);
    s.last_path = (int)path;
    s.last_tiles = tiles;
    s.last_blocks = blocks;
    if (path == exact_plan::SCHED_INSTALLED) {
        *sched = static_cast<const uint32_t*>(ctx->ws[WS_BLOCK_SCHED_HOOK]);
    } else if (path == exact_plan::SCHED_TABLE0 || path == exact_plan::SCHED_TABLE1) {
        const int h = path == exact_plan::SCHED_TABLE1;
        const exact_plan::SchedLayout l = exact_plan::sched_layout(call.n);
        AT_REQUIRE(s.layout_n == call.n && ctx->ws[WS_BLOCK_SCHED] && ctx->ws_bytes[WS_BLOCK_SCHED] >= 2 * l.bytes &&
                       l.blocks[exact_plan::sched_table_index(tiles)] == blocks,
                   "at_block_sched_pick: the tables are not those of n=%lld", (long long)call.n);
        const int rc = at_guard_enter(&s.guard[h], call.stream);   // (made on another stream: wait for it)
        if (rc) return rc;
        *sched = reinterpret_cast<const uint32_t*>(static_cast<const unsigned char*>(ctx->ws[WS_BLOCK_SCHED]) + (size_t)h * l.bytes +
                                                   l.table_off[exact_plan::sched_table_index(tiles)]);
        *half = h;
    }
    return AT_OK;
}

int at_block_sched_release(at_ctx* ctx, int half, hipStream_t stream) { return at_guard_leave(&ctx->sched.guard[half], stream); }

// Test hook: a caller-made schedule for the filter sweeps of exactly `blocks` row blocks (host array; it must be a
// permutation of [0, blocks): anything else would leave rows unanswered).  blocks = 0 removes it.  Waits for the device.
extern "C" int at_block_sched_install(at_ctx* ctx, const uint32_t* sched_host, int64_t blocks) {
    AT_REQUIRE(ctx && blocks >= 0 && blocks < (int64_t)UINT32_MAX && (sched_host || blocks == 0), "at_block_sched_install: bad arguments");
    AT_HIP(hipSetDevice(ctx->device));
    AT_HIP(hipDeviceSynchronize());   // no sweep is reading the schedule it replaces
    ctx->sched.installed_blocks = 0;
    if (blocks == 0) return AT_OK;
    std::vector<bool> seen((size_t)blocks, false);
    for (int64_t i = 0; i < blocks; i++) {
        const uint32_t b = sched_host[i];
        AT_REQUIRE((int64_t)b < blocks && !seen[b], "at_block_sched_install: not a permutation of [0, %lld) (entry %lld = %u)",
                   (long long)blocks, (long long)i, b);
        seen[b] = true;
    }
    void* dev = at_ws(ctx, WS_BLOCK_SCHED_HOOK, sizeof(uint32_t) * (size_t)blocks, nullptr);
    if (!dev) return AT_E_NOMEM;
    AT_HIP(hipMemcpy(dev, sched_host, sizeof(uint32_t) * (size_t)blocks, hipMemcpyHostToDevice));
    ctx->sched.installed_blocks = blocks;
    return AT_OK;
}

// Test hook: the table of blocks of `tiles` tiles (1, 2, 4) made beside `order` (the order_out of an at_visit_order_f32
// of n rows), copied to the caller's DEVICE buffer [ceil(ceil(n / 32) / tiles)] in stream order, with the tile weights
// (DEVICE bytes [ceil(n / 32)], may be null); *found = 0 and nothing copied when no table carries that tag.
extern "C" int at_block_sched_peek(at_ctx* ctx, const uint32_t* order, int64_t n, int tiles, uint32_t* table_out,
                                   unsigned char* weight_out, int* found, void* stream_) {
    AT_REQUIRE(ctx && order && n > 0 && table_out && found && exact_plan::sched_table_index(tiles) >= 0,
               "at_block_sched_peek: bad arguments");
    at_block_sched_state& s = ctx->sched;
    *found = 0;
    int h = -1;
    for (int i = 0; i < 2; i++)
        if (h < 0 && s.tag[i].valid && s.tag[i].order == order && s.tag[i].n == n) h = i;
    if (h < 0) return AT_OK;
    const exact_plan::SchedLayout l = exact_plan::sched_layout(n);
    AT_REQUIRE(s.layout_n == n && ctx->ws[WS_BLOCK_SCHED] && ctx->ws_bytes[WS_BLOCK_SCHED] >= 2 * l.bytes,
               "at_block_sched_peek: the tables are not those of n=%lld", (long long)n);
    AT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_;
    int rc = at_guard_enter(&s.guard[h], stream);
    if (rc) return rc;
    const unsigned char* base = static_cast<const unsigned char*>(ctx->ws[WS_BLOCK_SCHED]) + (size_t)h * l.bytes;
    const int t = exact_plan::sched_table_index(tiles);
    AT_HIP(hipMemcpyAsync(table_out, base + l.table_off[t], sizeof(uint32_t) * (size_t)l.blocks[t], hipMemcpyDeviceToDevice, stream));
    if (weight_out) AT_HIP(hipMemcpyAsync(weight_out, base + l.weight_off, (size_t)l.tiles, hipMemcpyDeviceToDevice, stream));
    rc = at_guard_leave(&s.guard[h], stream);
    if (rc) return rc;
    *found = 1;
    return AT_OK;
}

// Test hook: what the last filter sweep of the context started its blocks by (0 = visiting order, 1 = a table made
// beside its order, 2 = the installed schedule), its tiles per block and its number of blocks.  No device work.
extern "C" int at_block_sched_last(at_ctx* ctx, int* path, int* tiles, int64_t* blocks) {
    AT_REQUIRE(ctx && path, "at_block_sched_last: bad arguments");
    const int p = ctx->sched.last_path;
    *path = p == exact_plan::SCHED_IDENTITY ? 0 : p == exact_plan::SCHED_INSTALLED ? 2 : 1;
    if (tiles) *tiles = ctx->sched.last_tiles;
    if (blocks) *blocks = ctx->sched.last_blocks;
    return AT_OK;
}

// The row counts up to which an exact d = 64 sweep with the fused pre-pass runs one / two tiles per wave.  No device work.
extern "C" int at_block_sched_limits(int64_t* one_tile_max_rows, int64_t* two_tile_max_rows) {
    if (one_tile_max_rows) *one_tile_max_rows = exact_plan::ONE_TILE_MAX_ROWS;
    if (two_tile_max_rows) *two_tile_max_rows = exact_plan::TWO_TILE_MAX_ROWS;
    return AT_OK;
}

int at_filter_use_slot(at_ctx* ctx, int slot) {
    AT_REQUIRE(slot >= 0 && slot <= AT_FILTER_RING, "at_filter_use_slot: slot %d out of range", slot);
    at_filter_state& f = ctx->filter;
    if (!f.host_misc) {
        AT_HIP(hipHostMalloc(reinterpret_cast<void**>(&f.host_misc), (size_t)(AT_FILTER_RING + 1) * 128 * sizeof(unsigned),
                             hipHostMallocDefault));
        for (int s = 0; s <= AT_FILTER_RING; s++) f.ring[s].host_misc = f.host_misc + (size_t)s * 128;
    }
    at_filter_slot& fs = f.ring[slot];
    if (!fs.copied) AT_HIP(hipEventCreateWithFlags(&fs.copied, hipEventDisableTiming));
    fs.timed = 0;
    f.slot = slot;
    return AT_OK;
}

int at_filter_resolve_pending(at_ctx* ctx, bool wait_all) {
    at_filter_state& f = ctx->filter;
    while (f.count > 0) {
        at_filter_slot& fs = f.ring[f.head];
        if (wait_all) {
            AT_HIP(hipEventSynchronize(fs.copied));
        } else {
            const hipError_t q = hipEventQuery(fs.copied);
            if (q == hipErrorNotReady) break;   // an answer, not a failure (and the one code HIP does not keep pending)
            AT_HIP(q);
        }
        exact_plan::fold_ring_slot(f.tot, fs.host_misc, fs.rows);
        fold_timing(f, fs);
        f.head = (f.head + 1) % AT_FILTER_RING;
        f.count--;
    }
    return AT_OK;
}

extern "C" int at_assign_pruned_f32(at_ctx* ctx, const at_pruned_args* a, void* stream_) {
    AT_REQUIRE(ctx && a, "at_assign_pruned_f32: ctx / args is null");
    const int mode = a->guess_only ? 1 : 0;
    at_exact_call call{};
    call.x = a->x; call.n = a->n; call.d = a->d; call.c = a->c; call.k = a->k;
    call.order = a->order; call.hint_sorted = a->hint_sorted; call.cperm = a->cperm; call.ng = a->ng; call.dmin = a->bounds;
    call.ids = a->ids; call.dist = a->dist_or_null;
    call.stream = (hipStream_t)stream_;
    AT_REQUIRE(call.x && call.c && call.order && call.hint_sorted && call.cperm && (call.dmin || mode == 1) && call.ids,
               "at_assign_pruned_f32: null pointer");
    AT_REQUIRE(call.d == 64 || call.d == 128, "at_assign_pruned_f32: d must be 64 or 128");
    AT_REQUIRE(call.k > 0 && grouped_sizes_ok(call.n, 20, call.d, call.k, call.ng),
               "at_assign_pruned_f32: bad sizes n=%lld k=%d ng=%d", (long long)call.n, call.k, call.ng);
    AT_REQUIRE(at_aligned16(call.x) && at_aligned16(call.c), "at_assign_pruned_f32: x and c must be 16-byte aligned");
    AT_HIP(hipSetDevice(ctx->device));
    ctx->img16_trusted = a->image_current != 0;  // consumed (and cleared) by the filter sweep
    return exact_search(ctx, call, mode, a->prepass_done != 0, a->use_filter != 0);
}

// The pre-pass of at_assign_pruned_f32 on its own (per-row bound + per-tile group masks, kept in the
// context's workspace): lets a caller time or overlap it separately, then call
// at_assign_pruned_f32(..., prepass_done = 1) with the same arguments.
extern "C" int at_prune_mask_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k,
                                 const uint32_t* order, const uint32_t* hint_sorted, int ng, const float* dmin,
                                 int mode, void* stream_) {
    AT_REQUIRE(ctx && x && c && order && hint_sorted && (dmin || mode == 1), "at_prune_mask_f32: null pointer");
    AT_REQUIRE(grouped_sizes_ok(n, 20, d, k, ng), "at_prune_mask_f32: bad sizes");
    AT_HIP(hipSetDevice(ctx->device));
    at_exact_call call{};
    call.x = x; call.n = n; call.d = d; call.c = c; call.k = k;
    call.order = order; call.hint_sorted = hint_sorted; call.ng = ng; call.dmin = dmin;
    call.stream = (hipStream_t)stream_;
    const int rc = claim_prepass(ctx, call);
    if (rc) return rc;
    return at_prune_prepass(ctx, call, n, order, hint_sorted, mode);
}

// Test hook: what the preceding at_prune_mask_f32(n, ng) on this stream left in the workspace -- bd [n] and
// mask [ceil(n/32)][ceil(ng/32)] -- copied to the caller's device buffers, in stream order.  n and ng must be those of
// the last pre-pass that ran (another ng would read the masks with another stride).
extern "C" int at_prune_peek(at_ctx* ctx, int64_t n, int ng, float* bd_out, uint32_t* mask_out, void* stream_) {
    AT_REQUIRE(ctx && bd_out && mask_out && n > 0 && ng > 0, "at_prune_peek: bad arguments");
    const size_t bd_bytes = sizeof(float) * (size_t)n;
    const size_t mask_bytes = sizeof(uint32_t) * (size_t)((n + 31) / 32) * (size_t)((ng + 31) / 32);
    AT_REQUIRE(ctx->prepass_n == n && ctx->prepass_ng == ng, "at_prune_peek: the last pre-pass had n=%lld ng=%d, not n=%lld ng=%d",
               (long long)ctx->prepass_n, ctx->prepass_ng, (long long)n, ng);
    AT_REQUIRE(ctx->ws[WS_PRUNE_BD] && ctx->ws[WS_PRUNE_MASK] && ctx->ws_bytes[WS_PRUNE_BD] >= bd_bytes &&
                   ctx->ws_bytes[WS_PRUNE_MASK] >= mask_bytes,
               "at_prune_peek: workspace smaller than the pre-pass it records");
    AT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_;
    AT_HIP(hipMemcpyAsync(bd_out, ctx->ws[WS_PRUNE_BD], bd_bytes, hipMemcpyDeviceToDevice, stream));
    AT_HIP(hipMemcpyAsync(mask_out, ctx->ws[WS_PRUNE_MASK], mask_bytes, hipMemcpyDeviceToDevice, stream));
    return AT_OK;
}

extern "C" int at_filter_stats(at_ctx* ctx, int64_t* rows, int64_t* listed, double* sweep_ms, int64_t* sweeps,
                               int64_t* tiles, int64_t* refined, int reset) {
    AT_REQUIRE(ctx && rows && listed, "at_filter_stats: bad arguments");
    const int rcp = at_filter_resolve_pending(ctx, true);
    if (rcp) return rcp;
    at_filter_state& f = ctx->filter;
    *rows = f.tot.rows;
    *listed = f.tot.listed;
    if (sweep_ms) *sweep_ms = f.ms;
    if (sweeps) *sweeps = f.launches;
    if (tiles) *tiles = f.tot.tiles;
    if (refined) *refined = f.tot.refined;
    if (reset) {
        f.tot.rows = f.tot.listed = f.tot.tiles = f.tot.refined = f.launches = 0;
        f.ms = 0.0;
    }
    return AT_OK;
}

// Test hook: pre-pass + stage 1 only.  approx[2i] = approximate |c|^2 - 2 x.c of row i's winner,
// approx[2i+1] = gap to the runner-up; ids = the winners; *listed = rows the filter would hand to the
// fp32 sweep; tau_ab[0..1] = the coefficients of the acceptance threshold tau = a (|x|^2 + max|c|^2) + b.
extern "C" int at_filter_probe_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k,
                                   const uint32_t* order, const uint32_t* hint_sorted, const int32_t* cperm, int ng,
                                   const float* dmin, int64_t* ids, float* approx, int64_t* listed, void* stream_) {
    AT_REQUIRE(ctx && x && c && order && hint_sorted && cperm && dmin && ids && approx && listed,
               "at_filter_probe_f32: null pointer");
    AT_REQUIRE(k > 0 && grouped_sizes_ok(n, 20, d, k, ng), "at_filter_probe_f32: bad sizes");
    AT_HIP(hipSetDevice(ctx->device));
    at_exact_call call{};
    call.x = x; call.n = n; call.d = d; call.c = c; call.k = k;
    call.order = order; call.hint_sorted = hint_sorted; call.cperm = cperm; call.ng = ng; call.dmin = dmin;
    call.ids = ids;
    call.stream = (hipStream_t)stream_;
    int rc = claim_prepass(ctx, call);
    if (rc) return rc;
    rc = claim_filter(ctx, call);
    if (rc) return rc;
    rc = at_prune_prepass(ctx, call, n, order, hint_sorted, 0);
    if (rc) return rc;
    rc = at_filter_use_slot(ctx, AT_FILTER_RING);   // (a call outside the ring: the spare slot)
    if (rc) return rc;
    rc = at_filter_sweep(ctx, call, 1, false, nullptr, approx);
    if (rc) return rc;
    unsigned cnts[AT_AMB_SUBLISTS];
    AT_HIP(hipMemcpyAsync(cnts, call.misc + 64, sizeof cnts, hipMemcpyDeviceToHost, call.stream));
    AT_HIP(hipStreamSynchronize(call.stream));
    int64_t cnt = 0;
    for (unsigned s = 0; s < AT_AMB_SUBLISTS; s++) cnt += cnts[s];
    *listed = cnt;
    return AT_OK;
}

// Guess generator without a pre-sort, for rows whose own order is coherent (the frames of a clip follow
// one another): nearest of the ng group means -> the groups its neighbour table names -> best centroid
// among them, in one launch.  ids are guesses (feed at_visit_order_f32 / at_assign_pruned_f32), dist (optional)
// approximate distances.
extern "C" int at_assign_coarse_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k,
                                    const int32_t* cperm, int ng, const float* means, const uint32_t* gnbr,
                                    int64_t* ids, float* dist, void* stream_) {
    AT_REQUIRE(ctx && x && c && cperm && means && gnbr && ids, "at_assign_coarse_f32: null pointer");
    AT_REQUIRE(k > 0 && grouped_sizes_ok(n, 1, d, k, ng), "at_assign_coarse_f32: bad sizes");
    AT_REQUIRE(at_aligned16(x) && at_aligned16(c) && at_aligned16(means), "at_assign_coarse_f32: pointers must be 16-byte aligned");
    AT_HIP(hipSetDevice(ctx->device));
    return at_filter_coarse(ctx, x, n, d, c, k, cperm, ng, means, gnbr, ids, dist, (hipStream_t)stream_);
}
