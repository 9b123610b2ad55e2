// at_internal.h -- shared by the translation units of libaudio_tokens_amd.so (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/audio_tokens_amd.h"
#include "../../include/at_debug.h"
#include "exact_plan.h"

// Kernels that a caller may put on a stream of its own beside the k-means / tokenise sweeps (the pipeline computes the
// log-mel frames of later batches on the context's background stream) are compiled WITHOUT packed-fp32 vector
// instructions (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 / v_pk_mov_b32): Makefile, NOPK_OBJS.  Measured on gfx950
// (ROCm 7.2.0, round 3, profiles/r03_packed_fp32_beside_mfma.txt): while a wave of another kernel keeps the same SIMD's
// matrix pipe busy with back-to-back v_mfma_f32_32x32x16_f16 (the fp16 filter in guess mode: three products per tile), the
// packed ops of the 512-point log-mel kernel returned wrong values in lanes 48..63 of single registers -- 1.3e4 wrong
// frames of 1.0e7, always the frame owned by the wave's last 16 lanes, with either register allocation (223 / 190 VGPRs),
// with or without an s_waitcnt behind every LDS access, at 32 or 16 frames per block; the same source compiled without
// packed ops gave 0 wrong frames under the same load, at the same speed.  The form that fails (tools/pk_probe.py: one
// packed instruction per victim kernel, checked in place against the unpacked one) is v_pk_add_f32 with an op_sel half-swizzle
// of a vector-register source -- what the compiler emits for complex arithmetic; plain, negated, scalar- and constant-operand
// forms showed 0 mismatches in 1e11 operations each.  The sweeps' own packed ops have never differed
// from the dense reference (bench.py `verified`, tests/test_gpu_*) and produce the same guesses with and without, so the
// rule is applied to the producers only.  (A target("no-packed-fp32-ops") attribute on the kernels does the same but keeps
// the always-inline helpers from being inlined into them -- 30 calls and a scratch frame in the log-mel kernel --, and
// -Xarch_device -mno-packed-fp32-ops is accepted and ignored.)

// Workspace slots of a context (grown on demand, never shrunk).
enum at_ws_slot {
    WS_CENT_IMG = 0,   // assign: tiled/swizzled centroid image + |c|^2
    WS_SORT_KEYS_A,    // centroid_accum: keys / values, double buffered, + rocprim temp storage
    WS_SORT_KEYS_B,
    WS_SORT_VALS_A,
    WS_SORT_VALS_B,
    WS_SORT_TMP,
    WS_SEG_OFFSETS,    // centroid_accum: k+1 segment starts
    WS_REDUCE,         // at_sum_f32 / at_any_nonfinite partials
    WS_LOGMEL_FB,      // log-mel: banded filterbank tables
    WS_PRUNE_BD,       // pruned sweep: exact distance to the guess, per visiting position
    WS_PRUNE_MASK,     // pruned sweep: per 32-row tile, one bit per 32-centroid group
    WS_PRUNE_STATS,    // pruned sweep: {accumulators computed, accumulators of the dense sweep}
    WS_RESAMPLE_TAPS,  // resampler: polyphase filter taps [new][2*width + orig]
    WS_CENT_IMG16,     // fp16-split filter: centroid fragments (hi, lo) per group + |c|^2 + indices
    WS_FILTER_LIST,    // fp16-split filter: listed positions, sorted copy, order/hint of the redo pass
    WS_VISIT_KEYS_A,   // at_visit_order_f32: its own sort buffers (it may run while an accumulation still reads the others)
    WS_VISIT_KEYS_B,
    WS_VISIT_VALS_A,
    WS_VISIT_VALS_B,
    WS_VISIT_TMP,
    WS_CENT_IMG16B,    // fused coarse pass: fp16 image of the group means
    WS_IOTA,           // fused coarse pass: identity permutation of the means
    WS_FILTER_MISC,    // fp16-split filter: max|c|^2 bits, list length; running totals for at_filter_stats
    WS_PERM_RAW,       // at_rand_perm_prefix_device: draws, (position, step) sort buffers, links
    WS_PERM_KEYS_A,
    WS_PERM_KEYS_B,
    WS_PERM_VALS_A,
    WS_PERM_VALS_B,
    WS_PERM_TMP,
    WS_PERM_PREV,
    WS_PERM_LAST,
    WS_SPLIT_LIST,     // at_split_clusters_f32: the clusters that came out empty
    WS_TSTAT_IOTA,     // at_token_stats_f64: token ids before the sort, rocprim temp storage
    WS_TSTAT_TMP,
    WS_MT_RAW,         // at_mt_cached_draws: the resident start of the mt19937(1234) stream + the state behind it
    WS_LONG_PRED,      // centroid_accum: the long clusters of the last call (the next call's early set) + generation marks
    WS_LONG_EARLY,     // centroid_accum: block counts / bases and the member lists of the early set
    WS_LONG_LATE,      // centroid_accum: long clusters left to the pass behind the sort
    WS_BUCKETS,        // centroid_accum bucket path: counts, cursors, the list of long clusters
    WS_LOGMEL_ANY,     // log-mel, general n_fft: window, twiddles, banded filterbank
    WS_SUM_TICKET,     // at_sum_f32: arrival counter of its workgroups (the last one adds the partials up), zero between calls
    WS_ROW_FLAG,       // one int: a unit-row pass of at_logmel_f32 met a row whose squared norm is not finite
    WS_LOGMEL_MINMAX,  // at_logmel_minmax_f32, at_logmel_ragged_minmax_f32: per clip {min key, max key, NaN flag, pad}
    WS_FILTER_BLKSTATS, // fp16-split filter: one statistics record per workgroup of a sweep (switch filter_stats)
    WS_SILHOUETTE,     // at_silhouette_f32: sorted labels, permutation, segments, offsets, norms, rocprim temp storage
    WS_KNN_IMG,        // at_knn_f32: chunked centroid image (at_prep_chunked_image)
    WS_KNN,            // at_knn_f32 general path: keys of a block of rows (in, out), segment offsets, rocprim temp storage
    WS_RAGGED_TAPS0,   // at_mix_resample_ragged_f32: the taps of up to four reduced rate pairs (four consecutive slots)
    WS_RAGGED_TAPS1,
    WS_RAGGED_TAPS2,
    WS_RAGGED_TAPS3,
    WS_AVG_PRECISION,  // at_average_precision_f32 / at_ranking_metrics_f32: the two key buffers of a class chunk, tile records, tile partial sums
    WS_AVG_PRECISION_TMP,   // its rocprim temp storage
    WS_IP_IMG,         // at_assign_ip_f32: chunked centroid image (at_prep_chunked_image)
    WS_PQ_IMG,         // at_pq_encode_f32: MFMA-operand image of the M codebooks + their |c|^2 (pq.hip)
    WS_RQ_IMG,         // at_rq_encode_f32: chunked centroid image of the M stage codebooks (at_prep_chunked_image)
    WS_RQ_TMP,         // at_rq_encode_f32 general path: the running residual, when the caller takes none
    WS_MFCC_MAX,       // at_mfcc_f32 with top_db: one ordered key per clip, the maximum of its log-mel values (mfcc.hip)
    WS_MFCC_DCT,       // at_mfcc_f32 without a caller's table: the table of at_dct_matrix_host for (mfcc_dct_nmfcc, mfcc_dct_nmels)
    WS_WACC_KEYS_A,    // at_centroid_accum_weighted_f32: its own sort buffers (it never shares the unweighted accumulation's)
    WS_WACC_KEYS_B,
    WS_WACC_VALS_A,
    WS_WACC_VALS_B,
    WS_WACC_TMP,
    WS_WACC_SEG,       // ... its k+2 segment starts and the list of its long clusters
    WS_RQ_BEAM_RES,    // at_rq_beam_encode_f32: the two residual buffers [rows][B][d] of a block of rows
    WS_RQ_BEAM_LISTS,  // at_rq_beam_step_f32 / _encode_f32: the at_knn_f32 lists of one stage (ids, then distances)
    WS_RQ_BEAM_PATH,   // at_rq_beam_encode_f32: (parent, distance, word) of every slot of every stage of a block of rows
    WS_BLOCK_SCHED,    // at_visit_order_f32: the two halves of the block schedules (exact_plan.h SchedLayout), by call parity
    WS_BLOCK_SCHED_HOOK,   // at_block_sched_install: the caller's schedule
    WS_PQ_SEARCH_LISTS,    // at_pq_search_f32: the k smallest keys of every (query, slab) of a chunk of queries
    WS_IVF,                // at_ivf_build_f32 / at_ivf_search_f32: list counts and prefix sums; the pair table and the partial lists of a chunk of queries
    WS_IVFPQ,              // at_ivfpq_build / at_ivfpq_search_f32: list counts and prefix sums; the pair table and the partial lists of a chunk of queries
    WS_NSLOTS
};

// resampler tiling, shared by at_resample_f32, at_mix_resample_ragged_f32 and the plan that sizes the latter's launches
constexpr int AT_RS_RI = 4;              // accumulators per thread of the tiled kernel
constexpr int AT_RS_SEG_FLOATS = 8192;   // 32 KiB of LDS per workgroup
constexpr int AT_RS_COPY_PER_BLOCK = 4096;   // samples per workgroup where there is no filter

// Asynchronous exact calls leave their statistics words (and the events that time their stage-1 kernel) in a
// ring of slots; slots are folded into the totals when their copy has arrived -- polled, never waited for, unless
// the ring is full or a query asks for the totals (exact_search.cpp).
constexpr int AT_FILTER_RING = 64;
struct at_filter_slot {
    unsigned* host_misc;   // pinned, 128 words
    hipEvent_t copied;     // behind the D2H copy of the words
    hipEvent_t ev[2];      // around the stage-1 kernel (created on first use, and only under the switch filter_timing)
    int timed;             // both of ev[] were recorded by the call that holds this slot (else they are not read)
    int64_t rows;
};
// What a context keeps of the fp16-split filter between exact calls.
struct at_filter_state {
    exact_plan::Totals tot;      // rows swept / listed, tiles multiplied / refined; force_sync: a call whose list was long
                                 // switches the context to the synchronous form (with its fp32 MFMA redo) from then on
    double ms;                   // summed stage-1 kernel time, over `launches` launches
    int64_t launches;
    int slot;                    // the ring slot (or AT_FILTER_RING, the spare) the sweep being queued belongs to
    unsigned* host_misc;         // pinned, (AT_FILTER_RING + 1) x 128 words
    at_filter_slot ring[AT_FILTER_RING + 1];   // (the extra slot lends its timing events to the synchronous form)
    int head, count;             // oldest pending slot, number of pending slots
};

// Development switches (include/at_debug.h).  Read from the environment ONCE, in at_create -- never on a call
// path -- and changed afterwards only through at_debug_set.  Every one selects another route to the same bits
// (tests/test_gpu_ops.py::test_ab_switches_leave_the_bits_alone).
struct at_debug {
    int assign_variant;   // AT_ASSIGN_VARIANT   shape of the dense fp32 sweep (0 = default)
    int filter_fused;     // AT_FILTER_FUSED     1 = pre-pass inside the filter sweep (default), 0 = separate kernel
    int filter_sync;      // AT_FILTER_SYNC      1 = exact calls always take the synchronous form
    int prune_kernel;     // AT_PRUNE_KERNEL     0 = LDS-DMA form of the d = 64 fp32 pruned sweep
    int prune_nb;         // AT_PRUNE_NB         row tiles per wave of the fp32 pruned sweep (1, 2, 4; 0 = default)
    int filter_screen;    // AT_FILTER_SCREEN    0 = always evaluate all three fp16 products
    int filter_nb;        // AT_FILTER_NB        row tiles per wave of the filter sweep (1, 2, 4; 0 = by size)
    int filter_wps2;      // AT_FILTER_WPS2      1 = two waves per SIMD in the Lloyd-sized filter sweeps
    int dmin_kernel;      // AT_DMIN_KERNEL      0 = fp32 vector-ALU kernel for the centroid-to-group bounds
    int resample_simple;  // AT_RESAMPLE_SIMPLE  1 = one-thread-per-sample resampler
    int visit_bits;       // AT_VISIT_BITS       distance bits of the visiting-order key (0..8; default 8)
    int filter_stats;     // AT_FILTER_STATS     1 = the sweeps count accumulators / tiles for at_prune_stats, at_filter_stats
    int accum_buckets;    // AT_ACCUM_BUCKETS    0 = member lists by radix sort (the only form for k > 16 384)
    int logmel_fallback;  // AT_LOGMEL_FALLBACK  1 = Bluestein form of the log-mel transform for every n_fft that is not a power of two
    int ap_ws_mb;         // AT_AP_WS_MB         MiB the two key buffers of a class chunk of at_average_precision_f32 may take (default 1024; -m = chunks of m classes)
    int filter_timing;    // AT_FILTER_TIMING    1 = exact calls bracket their stage-1 kernel with two timing events (bench.py; off in the product)
    int block_sched;      // AT_BLOCK_SCHED      0 = the exact filter sweeps start their row blocks in visiting order
};

// What a log-mel table slot holds (WS_LOGMEL_FB: the tuned 512-point kernel's tables; WS_LOGMEL_ANY: every other
// n_fft's).  All zero = the slot holds nothing a call may use; fields a path does not use stay 0.
struct at_logmel_tables {
    int sr, nfft, nmels, hop, form;   // the key (hop: the 512 path's quad / plain decision depends on it; form: 0 power
                                      // of two, 1 mixed radix, 2 Bluestein)
    int nw, quads;                    // derived, 512 path: number of band weights, bands stored as 4-aligned quads
    float* user_copy;                 // malloc'd host copy of the caller's filterbank the tables were built from
                                      // (compared by value per call); null = the library's own filterbank
};
static inline void at_logmel_tables_clear(at_logmel_tables* t) {
    std::free(t->user_copy);
    *t = at_logmel_tables{};
}

// Workspace slots that belong to the context and are written by every call of an entry: two calls on different streams
// must not overlap in them, so a call on another stream than the previous one waits for it.
struct at_ws_guard {
    hipEvent_t ev;        // behind the last guarded call
    hipStream_t stream;   // ... which ran here
    int used;
};
enum at_guard_id {
    AT_GUARD_SUM = 0,   // at_sum_f32: WS_REDUCE partials, WS_SUM_TICKET
    AT_GUARD_SIL,       // at_silhouette_f32: WS_SILHOUETTE
    AT_GUARD_KNN,       // at_knn_f32: WS_KNN_IMG, WS_KNN
    AT_GUARD_AP,        // at_average_precision_f32 / at_ranking_metrics_f32: WS_AVG_PRECISION, WS_AVG_PRECISION_TMP
    AT_GUARD_IP,        // at_assign_ip_f32 sweep: WS_IP_IMG
    AT_GUARD_PQ,        // fused at_pq_encode_f32: WS_PQ_IMG
    AT_GUARD_RQ,        // at_rq_encode_f32: WS_RQ_IMG, WS_RQ_TMP
    AT_GUARD_MFCC,      // at_mfcc_f32 with top_db or without a caller's table: WS_MFCC_MAX, WS_MFCC_DCT
    AT_GUARD_WACC,      // at_centroid_accum_weighted_f32: WS_WACC_*
    AT_GUARD_RQ_BEAM,   // at_rq_beam_step_f32 / at_rq_beam_encode_f32: WS_RQ_BEAM_* (they call at_knn_f32, which takes
                        // AT_GUARD_KNN on the same stream inside: guards do not nest on one another's slots)
    AT_GUARD_PQ_SEARCH, // at_pq_search_f32: WS_PQ_SEARCH_LISTS
    AT_GUARD_IVF,       // at_ivf_build_f32 / at_ivf_search_f32: WS_IVF
    AT_GUARD_IVFPQ,     // at_ivfpq_build / at_ivfpq_search_f32: WS_IVFPQ
    AT_NGUARDS
};

// The block schedules of the exact filter sweeps (exact_plan.h: SchedLayout, sched_path).  at_visit_order_f32 call
// number j writes half j & 1 of WS_BLOCK_SCHED, so the table a running sweep reads -- that of the order before -- is not
// rewritten by a visit order that runs beside it on another stream.  Every user of a half, reader or writer, also goes
// through the half's guard (at_ws_guard: one event, one stream): it enters before it touches the half -- on another
// stream than the user before it, that is a wait for that user's leave event -- and leaves behind its last launch.  So
// the users of a half run one after the other in the order of their calls (contexts are used from one host thread), two
// sweeps over one order on two streams included: the second waits for the first, the next writer for the second.  A
// caller who strays from the Lloyd pattern waits, and never reads a torn table.  Both halves are laid out for one row
// count; a call with another n lays the slot out anew and drops what either half held.
struct at_block_sched_state {
    exact_plan::SchedTag tag[2];
    at_ws_guard guard[2];
    int64_t layout_n;          // the row count WS_BLOCK_SCHED is laid out for (0 = nothing)
    unsigned calls;            // at_visit_order_f32 calls that made tables
    int64_t installed_blocks;  // at_block_sched_install: blocks of the schedule in WS_BLOCK_SCHED_HOOK (0 = none)
    int last_path, last_tiles; // what the last filter sweep took (at_block_sched_last)
    int64_t last_blocks;
};

struct at_ctx {
    int device;
    at_debug dbg;
    void* ws[WS_NSLOTS];
    size_t ws_bytes[WS_NSLOTS];
    at_logmel_tables lm_fb, lm_any;   // what WS_LOGMEL_FB / WS_LOGMEL_ANY currently hold
    hipEvent_t mt_ready;   // behind the generation of WS_MT_RAW
    int mt_have;
    uint32_t mt_seed;
    int n_cus;             // multiProcessorCount of the device (read once in at_create)
    int rs_orig, rs_new;  // what WS_RESAMPLE_TAPS currently holds
    int rg_taps[4][2];    // what WS_RAGGED_TAPS0 .. 3 hold (rate pairs; 0 = nothing), replaced round robin
    int rg_next;
    at_filter_state filter;
    hipStream_t side_stream;             // centroid_accum: long member lists beside the short ones
    hipStream_t background_stream;       // at_background_stream: lowest priority, lent to the caller
    hipEvent_t side_ev[2];
    hipEvent_t side_ev2;                 // behind the segment offsets computed beside the sort (centroid_accum, radix path)
    int defer_join, join_pending;        // at_centroid_accum_defer / at_centroid_accum_join
    int buckets_k;                       // table size WS_BUCKETS was last zeroed for
    int long_pred_k;                     // table size WS_LONG_PRED was last used with
    unsigned long_gen;                   // generation of its 'summed early' marks
    // what at_group_min_dist_f32 left in WS_CENT_IMG16 / WS_FILTER_MISC[0]; a sweep may reuse it when its
    // caller vouches (prepass_done bit 1) that the centroids are unchanged
    const float* img16_c;
    const int32_t* img16_cperm;
    const unsigned* img16_misc;
    int img16_k, img16_d, img16_ng, img16_trusted;
    int img16_misc_clean;   // the words behind max|c|^2 in img16_misc are still zero (nobody has swept since they were cleared)
    // dynamic-LDS limits raised so far ON THIS DEVICE (hipFuncAttributeMaxDynamicSharedMemorySize is per device: a
    // process-wide "already raised" flag would leave the second device of a process at the default limit)
    struct { const void* func; size_t bytes; } lds_raised[48];
    int n_lds_raised;
    at_ws_guard guard[AT_NGUARDS];
    int mfcc_dct_nmfcc, mfcc_dct_nmels;   // what WS_MFCC_DCT holds (0 = nothing)
    int64_t prepass_n;                    // rows and groups of the last at_prune_prepass (what WS_PRUNE_BD / WS_PRUNE_MASK
    int prepass_ng;                       // hold; 0 = nothing): at_prune_peek refuses any other size
    at_block_sched_state sched;
};

// host.cpp.  enter: before the call touches the guarded slots (the event is created on first use, timing disabled; the
// stream waits only when it is not the one of the previous call); leave: behind everything the call queued.
int at_guard_enter(at_ws_guard* g, hipStream_t stream);
int at_guard_leave(at_ws_guard* g, hipStream_t stream);

// makes launches of `func` with `bytes` of dynamic LDS legal on the context's device (at most one runtime call per
// kernel and size step; nothing below the default limit)
int at_raise_lds(at_ctx* ctx, const void* func, size_t bytes);

int at_fail(int code, const char* fmt, ...);
// randperm.hip: resident prefix of the mt19937(seed) stream (6722 blocks of 624 outputs: covers the 4 194 304
// swaps of the largest subsample of BASELINE.json and ~500 cluster repairs at k = 8192)
constexpr int64_t AT_MT_CACHE_DRAWS = 624LL * 6722;
int at_mt_cached_draws(at_ctx* ctx, uint32_t seed, hipStream_t stream, const uint32_t** raw, int64_t* raw_n,
                       const uint32_t** state_end);
// Returns a device buffer of at least `bytes` for `slot` (contents undefined after growth).
void* at_ws(at_ctx* ctx, int slot, size_t bytes, hipStream_t stream);

// ---- error handling ----------------------------------------------------------------------------------------
// On ROCm 7.2 the error a failing HIP call leaves behind is STICKY: it stays in the calling thread until somebody
// calls hipGetLastError(), whatever succeeds in between (measured: tools/probes/event_probe.hip; hipErrorNotReady is
// the one code that is not kept).  Round 2 checked launches with a bare hipGetLastError() behind them, which
// therefore reported whatever any earlier call of this thread -- the library's, torch's, rocPRIM's -- had failed
// with and nobody had consumed ("kernel launch failed: invalid resource handle" out of a launch that was fine).
// Rules since round 3:
//   * every call whose failure is an error goes through AT_HIP: the call's OWN return code decides;
//   * every launch goes through AT_LAUNCH: hipLaunchKernel's OWN return code decides, never the thread's last error;
//   * a call whose failure is tolerated goes through AT_HIP_TOLERATE, which consumes the sticky error the failure
//     left (so it cannot surface in the host application's, or rocPRIM's, next hipGetLastError) and counts it;
//   * an error that is already pending when a launch is about to be made is not this library's launch failing:
//     it is consumed, counted and remembered (at_diag_*), and fails the call only under the switch strict_errors
//     ("stale error from an earlier call"), which the test-suite turns on.
struct at_diag_counters {
    long stale_seen;          // errors found pending in front of a launch
    int stale_last_code;
    const char* stale_last_file;
    int stale_last_line;
    long tolerated;           // failing calls whose failure was tolerated (AT_HIP_TOLERATE)
    int tolerated_last_code;
    const char* tolerated_last_file;
    int tolerated_last_line;
};
extern at_diag_counters g_at_diag;          // host.cpp (one per process; the counts are diagnostics, not state)
extern int g_at_strict_errors;              // host.cpp: switch strict_errors (AT_STRICT_ERRORS), process-wide

// host.cpp: tests for NaN / inf that a -ffast-math translation unit (host_group.cpp) can rely on
bool at_is_finite_f32(float v);
void at_zero_nonfinite_f32(float* v, size_t n);

hipError_t at_hip_tolerated(hipError_t e, const char* file, int line);
// returns hipSuccess, or -- strict mode -- the pending error
hipError_t at_stale_check(const char* file, int line);

#define AT_HIP(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            (void)hipGetLastError(); /* reported here: do not leave it pending as well */  \
            return at_fail(AT_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                            \
        }                                                                                  \
    } while (0)

// the call's code, with the sticky copy of a failure consumed and counted
#define AT_HIP_TOLERATE(expr) at_hip_tolerated((expr), __FILE__, __LINE__)

// Kernel launch by hipLaunchKernel, whose return value is this launch's own verdict.  Arguments are converted to the
// kernel's parameter types first (what the <<< >>> stub does), then passed by address.
template <typename... KArgs, typename... Args>
static inline hipError_t at_launch_raw(void (*kern)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                                       Args&&... args) {
    static_assert(sizeof...(KArgs) == sizeof...(Args), "at_launch_raw: argument count does not match the kernel's");
    std::tuple<KArgs...> params{static_cast<KArgs>(std::forward<Args>(args))...};
    void* ptrs[sizeof...(KArgs) > 0 ? sizeof...(KArgs) : 1];
    int i = 0;
    std::apply([&](auto&... p) { ((ptrs[i++] = const_cast<void*>(static_cast<const void*>(&p))), ...); }, params);
    return hipLaunchKernel(reinterpret_cast<const void*>(kern), grid, block, ptrs, lds, stream);
}

#define AT_LAUNCH(kern, grid, block, lds, stream, ...)                                                   \
    do {                                                                                                  \
        hipError_t s_ = at_stale_check(__FILE__, __LINE__);                                               \
        if (s_ != hipSuccess)                                                                             \
            return at_fail(AT_E_HIP, "stale error from an earlier call (pending before the launch of %s): %s (%s:%d)", \
                           #kern, hipGetErrorString(s_), __FILE__, __LINE__);                             \
        hipError_t e_ = at_launch_raw(kern, grid, block, lds, stream, __VA_ARGS__);                       \
        if (e_ != hipSuccess) {                                                                           \
            (void)hipGetLastError();                                                                      \
            return at_fail(AT_E_HIP, "launch of %s failed: %s (%s:%d)", #kern, hipGetErrorString(e_),     \
                           __FILE__, __LINE__);                                                           \
        }                                                                                                 \
    } while (0)

#define AT_REQUIRE(cond, ...)                                  \
    do {                                                       \
        if (!(cond)) return at_fail(AT_E_INVALID, __VA_ARGS__); \
    } while (0)

// at_raise_lds for a launch of `kernel` with `bytes` of dynamic LDS; returns its error from the calling function.
// (A template-id with commas goes in parentheses.)
#define AT_RAISE_LDS(ctx, kernel, bytes)                                                      \
    do {                                                                                       \
        const int rc_ = at_raise_lds(ctx, reinterpret_cast<const void*>(&kernel), bytes);      \
        if (rc_) return rc_;                                                                   \
    } while (0)

// ---- the exact pruned search (at_assign_pruned_f32): driver in exact_search.cpp, launches in prune.hip, filter.hip, assign.hip
// sub-lists of amb_cap slots each, arrays of at_amb_stride(n) words (AT_AMB_SUBLISTS: exact_plan.h)
static inline unsigned at_amb_cap(int64_t n) { return (unsigned)(n / AT_AMB_SUBLISTS + 128); }
static inline size_t at_amb_stride(int64_t n) { return (size_t)at_amb_cap(n) * AT_AMB_SUBLISTS; }

// One exact call: the caller's arguments, the workspace claimed for it and its stream.  The launches below read what
// they need from it; what varies between two launches of one call stays a parameter.
struct at_exact_call {
    const float* x;
    int64_t n;
    int d;
    const float* c;
    int k;
    const uint32_t* order;
    const uint32_t* hint_sorted;
    const int32_t* cperm;
    int ng;
    const float* dmin;
    int64_t* ids;
    float* dist;
    // claimed (exact_search.cpp): the fp32 image of the pruned sweep, the pre-pass outputs ...
    float* img;
    float* bd;          // exact distance to the guess, per visiting position
    uint32_t* mask;     // per 32-row tile, one bit per 32-centroid group (ngw words)
    int ngw;
    // ... and, for filtered calls, the statistics words and the five arrays of lstride words each
    unsigned* misc;     // 128 words: max|c|^2, statistics, sub-list lengths at [64 ..)
    uint32_t *list, *sorted, *order_amb, *hint_amb, *aux;
    unsigned amb_cap;
    size_t lstride;
    hipStream_t stream;
};

// prune.hip: per-row bound and per-tile group masks of the first n rows visited in `order` (the call's own, or the
// gathered list of a long redo), into call.bd / call.mask
int at_prune_prepass(at_ctx* ctx, const at_exact_call& call, int64_t n, const uint32_t* order, const uint32_t* hint_sorted,
                     int mode);
// assign.hip: WS_CENT_IMG claimed into call.img for the permuted fp32 image (one tile per group), the image built there,
// and the fp32 pruned sweep over n rows (kernel by d and the switches prune_nb / prune_kernel)
int at_pruned_image_claim(at_ctx* ctx, at_exact_call& call);
int at_pruned_image_build(at_ctx* ctx, const at_exact_call& call);
int at_pruned_sweep_f32(at_ctx* ctx, const at_exact_call& call, int64_t n, const uint32_t* order, const uint32_t* hint_sorted);
// filter.hip: stage 1 (collect: list the rows it cannot settle; fused_prepass: it computes call.bd and its own masks;
// dist_out: guess distances / a guess generator's approximate ones; approx_out: at_filter_probe_f32)
int at_filter_sweep(at_ctx* ctx, const at_exact_call& call, int collect, bool fused_prepass, float* dist_out,
                    float* approx_out);
// exact_search.cpp: the block order of a filter sweep of `blocks` row blocks of `tiles` tiles (exact_plan::sched_path):
// *sched = the table to start the blocks by, null = in visiting order; *half = the half of WS_BLOCK_SCHED it sits in
// (the stream has entered its guard: at_block_sched_release behind the launch), or -1
int at_block_sched_pick(at_ctx* ctx, const at_exact_call& call, bool exact_sweep, int tiles, int64_t blocks,
                        const uint32_t** sched, int* half);
int at_block_sched_release(at_ctx* ctx, int half, hipStream_t stream);
// ... the distance passes and the redo of the listed rows (m: list length, or the number of workgroups to launch)
int at_exact_dist_todo(at_ctx* ctx, const at_exact_call& call);
int at_exact_dist_rows(at_ctx* ctx, const at_exact_call& call);
int at_filter_redo_rows(at_ctx* ctx, const at_exact_call& call, int64_t m);
int at_filter_finish(at_ctx* ctx, const at_exact_call& call, int64_t redo_wgs);
// ... and the long-list redo: sub-lists -> contiguous (sorted, order_amb), then sorted and expanded to m >= m_valid rows
int at_amb_compact(at_ctx* ctx, const at_exact_call& call);
int at_filter_gather_ambiguous(at_ctx* ctx, const at_exact_call& call, int64_t m_valid, int64_t m);

// logmel.hip: the resident tables of a log-mel slot for `key` (sr, nfft, nmels, hop, form; the rest 0) and the caller's
// filterbank (device [nfft/2 + 1][nmels], compared by value) or the library's own (null); *tabs = the slot's device pointer.
// On a miss `build` makes the blob (at most cap_bytes) from the filterbank values on the host -- its head, then
// lmt::pack_bands (logmel_tables.h) -- and sets the derived fields of the record it is handed, a copy of the key.
typedef std::function<void(const float* fb, std::vector<float>& blob, at_logmel_tables* t)> at_logmel_builder;
int at_logmel_resident(at_ctx* ctx, int slot, at_logmel_tables* rec, const at_logmel_tables& key, size_t cap_bytes,
                       const float* fb_user_dev, hipStream_t stream, const at_logmel_builder& build, const float** tabs);

// center=True's reflect padding as an index into a clip of L samples: reflect, no edge repeat, then clamp (the clamp
// is only reachable for frames past T, which are never stored)
__device__ __forceinline__ long reflect_index(long q, long L) {
    if (q < 0) q = -q;
    if (q >= L) q = 2 * (L - 1) - q;
    if (q < 0) q = 0;
    if (q >= L) q = L - 1;
    return q;
}

// logmel_any.hip: every even n_fft other than 512, over the clips of a map (logmel_clips.h: lmc::UniformClips or
// lmc::PlanClips, the two instantiations) with n_frames output frames in all.
namespace lmc {
struct UniformClips;
struct PlanClips;
}
template <typename Clips>
int at_logmel_any(at_ctx* ctx, const Clips& clips, int64_t n_frames, int sample_rate, int n_fft, int hop, int n_mels,
                  const float* fb_user_dev, float* out, int frame_major, hipStream_t stream);

// assign.hip: builds the chunked centroid image of the any-d sweeps; its layout, at_chunked_image_tile_floats(d, na) and
// the sweep over it that knn.hip, ip.hip and rq.hip share are in chunked_sweep.h.
int at_prep_chunked_image(at_ctx* ctx, const float* c, int k, int d, int na, float* img, hipStream_t stream);

int at_group_min_dist_f16(at_ctx* ctx, const float* c, int k, int d, const int32_t* cperm, int ng, float* dmin,
                          hipStream_t stream);

int at_filter_coarse(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k, const int32_t* cperm, int ng,
                     const float* means, const uint32_t* gnbr, int64_t* ids, float* dist, hipStream_t stream);

// exact_search.cpp.  wait_all: fold every pending slot (blocking); otherwise only those whose copy has already arrived
int at_filter_resolve_pending(at_ctx* ctx, bool wait_all);
// the sweep queued next belongs to ring slot `slot` (AT_FILTER_RING: the spare, for calls outside the ring); creates
// what the slot needs on first use and marks its timing events as not recorded
int at_filter_use_slot(at_ctx* ctx, int slot);

static inline bool at_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// unit rows with a verdict: *bad (device int, may be null) is set when a row's norm is not finite (l2norm.hip)
int at_l2norm_rows_flagged(at_ctx* ctx, const float* x, int64_t n, int d, float* y, int* bad, hipStream_t stream);
int* at_row_flag(at_ctx* ctx, hipStream_t stream);   // the context's flag word (WS_ROW_FLAG), cleared when first allocated

