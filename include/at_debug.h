/*
 * at_debug.h -- development and test hooks of libaudio_tokens_amd.so.  NOT part of the operator surface
 * (include/audio_tokens_amd.h): nothing a binding of the reference's operators needs is declared here.
 *
 *   at_debug_set / at_debug_get   A/B switches of a context.  Each selects another route to the SAME bits
 *                                 (another kernel shape, a separate pre-pass, the synchronous form ...).  They are
 *                                 initialised from the AT_* environment variables once, in at_create, and never read
 *                                 from the environment again; names:
 *                                   assign_variant filter_fused filter_sync prune_kernel prune_nb filter_screen
 *                                   filter_nb filter_wps2 dmin_kernel resample_simple accum_buckets filter_stats visit_bits
 *                                   filter_timing logmel_fallback ap_ws_mb block_sched strict_errors
 *                                 (logmel_fallback = 1 is the one switch that does NOT keep the bits: the even n_fft that
 *                                 are not powers of two all take the Bluestein form of the transform, so that it can be
 *                                 held against the mixed-radix form at the sizes that have both; same tolerance)
 *                                 (filter_stats = 1 makes the fp16-split sweeps count for the two calls below: one record
 *                                 per workgroup and a small reduction kernel behind every sweep; off by default)
 *                                 (ap_ws_mb: the MiB the two key buffers of a class chunk of at_average_precision_f32
 *                                 may take, default 1024; a negative value -m asks for chunks of exactly m classes; any
 *                                 value gives the same bits, in more or fewer chunks)
 *                                 filter_timing = 1 brackets the stage-1 kernel of every exact call with two timing events
 *                                 (what at_filter_stats' sweep_ms sums; bench.py turns it on, the product leaves it off);
 *                                 strict_errors (process-wide, also AT_STRICT_ERRORS): a HIP error found pending in the
 *                                 calling thread in front of one of the library's launches fails the call ("stale error
 *                                 from an earlier call") instead of being consumed and counted
 *                                 block_sched = 0: at_visit_order_f32 makes no block schedules and the exact filter sweeps
 *                                 start their row blocks in visiting order (default 1: widest need sets first);
 *   at_diag_errors                what the library met and did not treat as its own failure: errors pending in front of a
 *                                 launch (somebody's earlier call failed and nobody consumed the error) and failures it
 *                                 tolerates by design; counts, last codes and source positions.  No device work.
 *   at_debug_leave_error_pending  test hook: makes a HIP call fail without consuming its error, as a swallowed return code does
 *   at_prune_stats                running totals over the context's exact pruned sweeps: 32x32 accumulators computed /
 *                                 accumulators of the dense sweep.  Synchronises the device; reset != 0 clears them.
 *   at_filter_stats               fp16-split filter: rows swept / rows handed to the fp32 redo, the summed HIP-event
 *                                 time of the stage-1 kernel over `sweeps` exact calls, 32x32 tiles multiplied hi*hi /
 *                                 refined with the lo products (NULL skips a field).  Waits for the calls in flight.
 *   at_filter_probe_f32           stage 1 of an exact call only: approx[2i], approx[2i+1] = approximate |c|^2 - 2 x.c
 *                                 of row i's winner and its gap to the runner-up; *listed = rows it would hand on.
 *   at_prune_peek                 test hook: bd [n] and mask [ceil(n/32)][ceil(ng/32)] as the preceding at_prune_mask_f32
 *                                 (same n, ng, same stream) left them in the workspace, copied to DEVICE buffers.
 *   at_block_sched_install        test hook: a caller-made block schedule (HOST array) for the exact filter sweeps of exactly
 *                                 `blocks` row blocks, until blocks = 0 removes it; refused unless it is a permutation of
 *                                 [0, blocks).  Waits for the device.
 *   at_block_sched_peek           test hook: the table of blocks of `tiles` 32-row tiles (1, 2, 4) that at_visit_order_f32
 *                                 made beside `order` (its order_out, n rows), and the tile weights (bytes, may be NULL),
 *                                 copied to DEVICE buffers in stream order; *found = 0 when no table carries that tag.
 *   at_block_sched_last           what the context's last filter sweep started its blocks by: 0 visiting order, 1 a table
 *                                 made beside its order, 2 the installed schedule; its tiles per block and block count.
 *   at_block_sched_limits         the row counts up to which an exact d = 64 sweep runs one / two tiles per wave.
 *   at_waccum_limits              the member-list lengths at which at_centroid_accum_weighted_f32 changes its path: rows
 *                                 per register set of the one-wave kernel (lanes with 1 or 2 features / with 4), the
 *                                 longest list that kernel walks (longer ones go to the feature-sliced kernel) and the
 *                                 members per buffer of that kernel's LDS ring (NULL skips a field).  No device work.
 *   at_pq_search_limits           the seams of at_pq_search_f32 for a call with M sub-spaces, ntotal database rows and k
 *                                 places: queries per workgroup (4 up to M = 32, 2 above), database rows per slab, and
 *                                 the queries whose lists fill the workspace budget -- a call with more takes them in
 *                                 chunks of that many (NULL skips a field).  No device work.
 *   at_ivfpq_search_limits        the seams of at_ivfpq_search_f32 for a call with M sub-spaces, nprobe probes per query
 *                                 and k places: (query, probe) pairs per workgroup (4 up to M = 32, 2 above), the rows a
 *                                 list of the image is padded to, and the queries whose partial lists fill the workspace
 *                                 budget -- a call with more takes them in chunks of that many (NULL skips a field).  No
 *                                 device work.
 */
#ifndef AUDIO_TOKENS_AMD_DEBUG_H
#define AUDIO_TOKENS_AMD_DEBUG_H

#include "audio_tokens_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int at_debug_set(at_ctx* ctx, const char* name, int value);
int at_debug_get(const at_ctx* ctx, const char* name, int* value);
int at_diag_errors(int64_t* stale_seen, int* stale_last_code, int64_t* tolerated, int* tolerated_last_code, char* where,
                   int where_bytes, int reset);
int at_debug_leave_error_pending(void);

int at_prune_stats(at_ctx* ctx, int64_t* needed_host, int64_t* total_host, int reset);
int at_filter_stats(at_ctx* ctx, int64_t* rows, int64_t* listed, double* sweep_ms, int64_t* sweeps,
                    int64_t* tiles, int64_t* refined, int reset);
int at_filter_probe_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k,
                        const uint32_t* order, const uint32_t* hint_sorted, const int32_t* cperm, int ng,
                        const float* dmin, int64_t* ids, float* approx, int64_t* listed, void* stream);
int at_prune_peek(at_ctx* ctx, int64_t n, int ng, float* bd_out, uint32_t* mask_out, void* stream);
int at_block_sched_install(at_ctx* ctx, const uint32_t* sched_host, int64_t blocks);
int at_block_sched_peek(at_ctx* ctx, const uint32_t* order, int64_t n, int tiles, uint32_t* table_out,
                        unsigned char* weight_out, int* found, void* stream);
int at_block_sched_last(at_ctx* ctx, int* path, int* tiles, int64_t* blocks);
int at_block_sched_limits(int64_t* one_tile_max_rows, int64_t* two_tile_max_rows);
int at_waccum_limits(int* short_batch, int* short_batch_wide, int* long_list, int* ring_chunk);
int at_pq_search_limits(int* queries_per_block, int* slab_rows, int64_t* queries_per_chunk, int M, int64_t ntotal, int k);
int at_ivfpq_search_limits(int* pairs_per_block, int* rows_per_group, int64_t* queries_per_chunk, int M, int nprobe, int k);

#ifdef __cplusplus
}
#endif
#endif /* AUDIO_TOKENS_AMD_DEBUG_H */
