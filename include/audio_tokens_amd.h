/*
 * audio_tokens_amd.h -- C ABI of the MI355X (gfx950) audio-tokenisation hot path.
 *
 * The reference (danavery/audio-tokens) has no FFI of its own: its three stage classes call two
 * third-party operators directly.  The entry points below are what a native replacement of those
 * operators binds; each cites the reference call site it stands in for (paths relative to the
 * reference repository).
 *
 *   torchaudio.transforms.MelSpectrogram(...)(wave) -> AmplitudeToDB()      at_logmel_f32
 *       processors/spectrogram_generator.py:28-34, 123-126
 *   torchaudio.transforms.Resample(sr, 22050)(wave)                        at_resample_f32
 *       processors/spectrogram_generator.py:117-121
 *   torchaudio.load(path) of a .flac file                                  at_flac_index_host,
 *       processors/spectrogram_generator.py:99                             at_flac_decode_f32
 *   np.linalg.norm(axis=1) row normalisation                               at_l2norm_rows_f32
 *       processors/cluster_creator.py:64-66, processors/spec_tokenizer.py:106-109
 *   faiss.IndexFlatL2(d).add(c); .search(x, 1)                             at_assign_f32
 *       processors/spec_tokenizer.py:77, 123-127 (and inside faiss.Kmeans.train)
 *   faiss.IndexFlatL2(d).search(x, k), k >= 2 (not used by the reference)  at_knn_f32
 *   faiss.IndexFlatIP(d).search(x, 1), Kmeans(spherical=True) (likewise)   at_assign_ip_f32, at_renorm_rows_f32
 *   faiss.ProductQuantizer(d, M, 8).compute_codes(x) / .decode(codes) (likewise)  at_pq_encode_f32, at_pq_decode_f32
 *   faiss.IndexPQ(d, M, 8).search(x, k) over stored codes (likewise; the library's own contract)  at_pq_search_f32
 *   faiss.IndexIVFFlat(quantizer, d, nlist).search(x, k) (likewise; the library's own contract)  at_ivf_build_f32, at_ivf_search_f32
 *   faiss.IndexIVFPQ(quantizer, d, nlist, M, 8).search(x, k) (likewise; the library's own contract)  at_ivfpq_build, at_ivfpq_search_f32
 *   greedy residual quantiser (RVQ, beam 1; the library's own contract)    at_rq_encode_f32, at_rq_decode_f32
 *   beam-search residual quantiser (beam 1 .. 32; the library's own contract)  at_rq_beam_step_f32, at_rq_beam_encode_f32
 *   torchaudio.transforms.MFCC / ComputeDeltas on log-mel rows (likewise)  at_mfcc_f32, at_deltas_f32,
 *                                                                          at_dct_matrix_host
 *   faiss.Kmeans(d, k, niter).train(x, init_centroids)                     at_rand_perm_mt19937,
 *       processors/cluster_creator.py:42-56                                at_gather_rows_f32,
 *                                                                          at_assign_f32, at_assign_hinted_f32,
 *                                                                          at_centroid_accum_f32,
 *                                                                          at_centroid_accum_weighted_f32,
 *                                                                          at_centroid_finalize_f32,
 *                                                                          at_split_clusters_host,
 *                                                                          at_sum_f32
 *
 * Conventions
 *   - plain C: raw pointers and sizes, no C++/torch types.  Every `const float*`/`float*` named
 *     x, c, wave, out, sums ... is a DEVICE pointer on the context's GPU unless the function name
 *     ends in _host or the parameter says (host).  `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream).  All device work is enqueued on that stream and is not
 *     synchronised unless stated.
 *   - the caller owns every buffer it passes; the library owns only the workspace behind
 *     at_ctx (grown on demand, freed by at_destroy).  A context is bound to one device and is
 *     not re-entrant: use one per host thread / stream.
 *   - return value: 0 = ok, negative = error (AT_E_*); at_last_error() gives the message of the
 *     calling thread's last failure.  Nothing throws across this boundary.
 */
#ifndef AUDIO_TOKENS_AMD_H
#define AUDIO_TOKENS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AT_VERSION 100 /* 0.1.0 */

#define AT_OK 0
#define AT_E_INVALID (-1)  /* bad argument (null pointer, size, unsupported shape) */
#define AT_E_HIP (-2)      /* a HIP runtime call failed */
#define AT_E_NOMEM (-3)    /* workspace allocation failed */
#define AT_E_TOO_FEW (-4)  /* faiss: "Number of training points should be at least ..." */
#define AT_E_NONFINITE (-5)/* faiss: "input contains NaN's or Inf's" */
#define AT_E_COMM (-6)     /* RCCL is not available in the process, or a collective failed */

/* at_logmel_f32 output layouts */
#define AT_LAYOUT_MEL_MAJOR 0   /* out[clip][n_mels][T]  -- the reference's .npy file layout */
#define AT_LAYOUT_FRAME_MAJOR 1 /* out[clip*T + t][n_mels] -- what ClusterCreator/SpecTokenizer
                                   build with np.load(f).T + np.concatenate */

typedef struct at_ctx at_ctx;

/* ---- context -------------------------------------------------------------------------------- */
int at_version(void);
const char* at_last_error(void);
int at_create(int device, at_ctx** out);
void at_destroy(at_ctx* ctx);
/* bytes of device workspace currently held by the context */
int64_t at_workspace_bytes(const at_ctx* ctx);
/* A stream of the LOWEST priority the device offers, owned by the context (created on first use, destroyed by
 * at_destroy): for work that should fill the gaps of the caller's main stream without delaying it -- the pipeline
 * computes the log-mel frames of the k-means batches to come there while the batch before them is trained
 * (cluster_creator.py:42-56 loads batch by batch too).  *stream_out is a hipStream_t. */
int at_background_stream(at_ctx* ctx, void** stream_out);

/* ---- host helpers (no GPU work) --------------------------------------------------------------*/
/* faiss utils/random.cpp rand_perm(perm, n, seed): std::mt19937 Fisher-Yates. perm: host [n]. */
int at_rand_perm_mt19937(int64_t n, int64_t seed, int32_t* perm_host);
/* The first m entries of that same permutation (m <= n) without running the remaining n-m
 * Fisher-Yates steps, which cannot touch them.  prefix_host: host [m]. */
int at_rand_perm_prefix_mt19937(int64_t n, int64_t seed, int64_t m, int32_t* prefix_host);
/* torchaudio.functional.melscale_fbanks(n_fft/2+1, 0, sr//2, n_mels, sr, norm=None, "htk").
 * fb_host: [n_fft/2+1][n_mels]. */
int at_mel_filterbank_host(int sample_rate, int n_fft, int n_mels, float* fb_host);
/* number of STFT frames of an L-sample clip with center=True: 1 + L / hop */
int64_t at_num_frames(int64_t L, int hop);
/* faiss Clustering.cpp split_clusters(d, k, n, 0, hassign, centroids) on HOST buffers
 * (hassign [k], centroids [k][d]); *nsplit receives the number of re-seeded clusters. */
int at_split_clusters_host(int d, int k, int64_t n, float* hassign_host, float* centroids_host,
                           int* nsplit);

/* ---- device operators ------------------------------------------------------------------------*/
/* Fused STFT -> |.|^2 -> mel -> 10*log10(max(.,1e-10)).
 *   wave: n_clips clips of L samples, clip i at wave + i*wave_stride (floats).
 *   fb_or_null: DEVICE [n_fft/2+1][n_mels] filterbank, or NULL = the library's own
 *   (at_mel_filterbank_host values).  n_fft: every EVEN size from 64 to 4096 (512, the reference's default, takes
 *   the tuned kernel; the other powers of two radix-8 Stockham passes; n_fft/2 = 2^a 3^b 5^c 7^d -- 400, 480, 1000,
 *   ... -- mixed-radix passes; every other even size Bluestein's chirp transform).  Odd sizes are rejected: torch
 *   counts 1 + (L - 1) / hop frames for them and at_num_frames has no n_fft argument.  1 <= hop <= n_fft.
 *   out: n_clips*n_mels*T floats in `layout`.  fuse_l2norm != 0 (frame-major only) additionally
 *   applies at_l2norm_rows_f32 to every frame before it is stored. */
int at_logmel_f32(at_ctx* ctx, const float* wave, int64_t n_clips, int64_t L, int64_t wave_stride,
                  int sample_rate, int n_fft, int hop, int n_mels, const float* fb_or_null,
                  float* out, int layout, int fuse_l2norm, void* stream);

/* torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults (sinc_interp_hann,
 * lowpass_filter_width 6, rolloff 0.99) -- processors/spectrogram_generator.py:117-121.
 * out: n_clips rows of at_resample_length(L, ...) samples, row stride out_stride floats.
 * at_resample_taps_host builds the polyphase taps [new][2*width + orig] on the host (pass
 * taps_host = NULL to query orig/new/width only). */
int64_t at_resample_length(int64_t L, int orig_freq, int new_freq);
int at_resample_taps_host(int orig_freq, int new_freq, int* orig_out, int* new_out, int* width_out,
                          float* taps_host, int64_t taps_capacity);
int at_resample_f32(at_ctx* ctx, const float* wave, int64_t n_clips, int64_t L, int64_t wave_stride,
                    int orig_freq, int new_freq, float* out, int64_t out_stride, void* stream);

/* y[i] = x[i] / (||x[i]||_2 + 1e-10), fp32, numpy's pairwise summation order (bit-exact with
 * numpy for finite inputs).  x == y is allowed. */
int at_l2norm_rows_f32(at_ctx* ctx, const float* x, int64_t n, int d, float* y, void* stream);

/* SpectrogramGenerator.normalize_spectrogram (processors/spectrogram_generator.py:129-131, config.normalize):
 * every clip of clip_elems floats (a [n_mels][T] spectrogram) becomes (x - min) / (max - min), in place, with torch's
 * fp32 operations (same bits as the reference's torch expression). */
int at_minmax_scale_clips_f32(at_ctx* ctx, float* x, int64_t n_clips, int64_t clip_elems, void* stream);

/* ClusterCreator.apply_convolution / SpecTokenizer.apply_convolution (processors/cluster_creator.py:68-81,
 * processors/spec_tokenizer.py:92-104,115-121; config.use_convolution): nn.Conv1d(1, num_kernels, kernel_size,
 * padding = (kernel_size - 1) / 2) along the mel axis of every frame.  x: [n][n_mels]; weight: DEVICE
 * [num_kernels][kernel_size] (the module's weight[:, 0, :]); bias_or_null: DEVICE [num_kernels];
 * out: [n][n_mels * num_kernels] with feature = mel * num_kernels + kernel (the reference's transpose + reshape).
 * out(m, j) = fma chain over the taps in ascending order, started from the bias. */
int at_conv1d_mel_f32(at_ctx* ctx, const float* x, int64_t n, int n_mels, const float* weight, const float* bias_or_null,
                      int num_kernels, int kernel_size, int padding, float* out, void* stream);

/* generate_mel_spectrogram followed by normalize_spectrogram (processors/spectrogram_generator.py:123-131 with
 * config.normalize = True) for a batch of clips: at_logmel_f32(..., fuse_l2norm = 0) and at_minmax_scale_clips_f32
 * in one call, same bits.  The log-mel kernel collects every clip's extremes while a computed block is still in LDS,
 * so the scaling costs one pass over the spectrogram instead of a reduction pass plus a scaling pass.  At most
 * 65535 clips per call. */
int at_logmel_minmax_f32(at_ctx* ctx, const float* wave, int64_t n_clips, int64_t L, int64_t wave_stride,
                         int sample_rate, int n_fft, int hop, int n_mels, const float* fb_or_null,
                         float* out, int layout, void* stream);

/* ---- ragged front end: mono mix, resampler and log-mel for clips of any length, channel count and rate -----------
 * What SpectrogramGenerator.populate_specs does per clip (convert_to_mono, resample, generate_mel_spectrogram:
 * processors/spectrogram_generator.py:105-126), for a whole batch of unequal clips with one launch per rate pair
 * present and one log-mel launch.  Same bits as at_resample_f32 then at_logmel_f32 on each clip alone.
 *
 * at_frontend_plan_host (no GPU work) lays the batch out.  Input: one at_frontend_clip_in per clip -- its [C][L]
 * block starts `offset` floats into the input buffer, rows `row_stride` floats apart; C is 1 or 2 (more channels are
 * mixed by the caller and enter as mono).  Output:
 *   plan[n_clips]    one record per clip: resampled length, where its mono row lies in the intermediate buffer (a
 *                    multiple of 4 floats, so 16-byte loads apply), its frames T = at_num_frames(out_length, hop) and
 *                    first output frame (exclusive prefix sum), its group, and the prefixes the kernels search to go
 *                    from a block or frame number to the clip.  A clip with out_length <= n_fft/2 is too short for
 *                    the reflect padding: too_short = 1, no frames.
 *   order[n_clips]   clip indices sorted by group (stable); group g owns order[first .. first + count).
 *   groups           one record per reduced rate pair (orig/g, new/g), in order of first appearance: 44100 -> 22050
 *                    and 48000 -> 24000 are one group.  Clips already at common_sr form a group with no filter.
 *                    *totals.n_groups receives the number of groups; more than groups_capacity is an error.
 *   totals           int64 sums: floats of the intermediate buffer, frames, blocks, too-short clips.
 * The plan is uploaded as it is (plan and order) and handed to the two device calls, which trust it. */
typedef struct at_frontend_clip_in {
    int64_t offset, row_stride, length;
    int32_t channels, rate;
} at_frontend_clip_in;

typedef struct at_frontend_clip {
    int64_t in_offset, in_row_stride, in_length;
    int64_t out_length;       /* at_resample_length(in_length, rate, common_sr) */
    int64_t mono_offset;      /* floats into the intermediate buffer, a multiple of 4 */
    int64_t first_frame;      /* exclusive prefix sum of n_frames */
    int64_t first_block16;    /* exclusive prefix sums of ceil(n_frames / 16) and ceil(n_frames / 32): the tuned */
    int64_t first_block32;    /*   n_fft = 512 kernel works on blocks of 16 or 32 frames of one clip */
    int64_t rs_first_block;   /* exclusive prefix sum, within the group, of the clip's resampler blocks */
    int32_t n_frames;         /* 0 when too short */
    int32_t channels, group, too_short;
} at_frontend_clip;

#define AT_FRONTEND_COPY 0    /* no filter: copy or mix */
#define AT_FRONTEND_SIMPLE 1  /* one thread per output sample */
#define AT_FRONTEND_TILED 2   /* input span staged in LDS (what at_resample_f32 uses whenever it fits) */

typedef struct at_frontend_group {
    int64_t first, count;     /* slice of order[] */
    int64_t n_blocks;         /* workgroups of the group's launch */
    int64_t out_per_block;    /* output samples per workgroup */
    int32_t orig_freq, new_freq;   /* the rate pair of the group's first clip, as given */
    int32_t orig, nw;         /* reduced by their gcd */
    int32_t width, K;         /* filter half width and taps per phase; 0 with no filter */
    int32_t mode, TI;         /* AT_FRONTEND_*; TILED: input steps per workgroup */
} at_frontend_group;

typedef struct at_frontend_totals {
    int64_t mono_floats, n_frames, n_blocks16, n_blocks32, n_short, n_groups;
} at_frontend_totals;

int at_frontend_plan_host(const at_frontend_clip_in* clips, int64_t n_clips, int common_sr, int n_fft, int hop,
                          at_frontend_clip* plan, int32_t* order, at_frontend_group* groups, int64_t groups_capacity,
                          at_frontend_totals* totals);

/* One group of a plan: every clip of it is read from in + in_offset ([C][L], C = 1 passes through, C = 2 is
 * (l + r) * 0.5f, torch.mean's bits), resampled with at_resample_f32's arithmetic (tap order included) and written to
 * mono + mono_offset.  plan_dev, order_dev: DEVICE copies of the plan's arrays; group: the HOST record.  One launch. */
int at_mix_resample_ragged_f32(at_ctx* ctx, const float* in, const at_frontend_clip* plan_dev, const int32_t* order_dev,
                               const at_frontend_group* group, float* mono, void* stream);

/* at_logmel_f32 for all clips of a plan in one launch: clip i is mono + mono_offset, out_length samples, reflected at
 * its own edges.  Every n_fft, hop, n_mels and filterbank at_logmel_f32 accepts.  out: mel-major, clip i is a
 * contiguous [n_mels][n_frames] block at n_mels * first_frame floats; frame-major, [totals.n_frames][n_mels] (with or
 * without fuse_l2norm).  bad: int32 [n_clips], non-zero where a value stored for the clip is NaN or +-Inf.
 * totals: the HOST record of the plan.  No limit of 65535 clips. */
int at_logmel_ragged_f32(at_ctx* ctx, const float* mono, const at_frontend_clip* plan_dev, int64_t n_clips,
                         const at_frontend_totals* totals, int sample_rate, int n_fft, int hop, int n_mels,
                         const float* fb_or_null, float* out, int layout, int fuse_l2norm, int32_t* bad, void* stream);

/* at_logmel_ragged_f32 followed by normalize_spectrogram (processors/spectrogram_generator.py:129-131, config.normalize)
 * on every clip of the plan: clip i's block holds (spec - min_i) / (max_i - min_i), torch's bits (two fp32 subtractions
 * and one IEEE division per value); a NaN anywhere in a clip makes the whole clip NaN.  Same arguments.  The extremes
 * are collected by the tuned kernel itself at n_fft = 512 and by a reduction pass over the output at every other size;
 * one scaling pass follows.  fuse_l2norm (frame-major): at_l2norm_rows_f32 over the SCALED rows, in place.
 * bad: non-zero where a value stored for the clip is NaN or +-Inf AFTER the scaling, which is where the reference
 * checks: a constant clip (digital silence: 0 / 0) is flagged like a clip with a NaN sample.  No limit of 65535 clips. */
int at_logmel_ragged_minmax_f32(at_ctx* ctx, const float* mono, const at_frontend_clip* plan_dev, int64_t n_clips,
                                const at_frontend_totals* totals, int sample_rate, int n_fft, int hop, int n_mels,
                                const float* fb_or_null, float* out, int layout, int fuse_l2norm, int32_t* bad,
                                void* stream);

/* Nearest centroid under squared L2 (IndexFlatL2.search(x, 1)):
 *   dis(i,j) = max(0, (|x_i|^2 + |c_j|^2) - 2 <x_i, c_j>), all fp32, inner products and norms as
 *   ascending-index fmaf chains (v_mfma_f32_32x32x2_f32); ids[i] = lowest j attaining the minimum.
 *   n < 20 uses faiss's small-batch form sum (x-c)^2 instead (distance_compute_blas_threshold).
 *   ids: int64 [n]; dist_or_null: float [n]. */
int at_assign_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k,
                  int64_t* ids, float* dist_or_null, void* stream);

/* The same answer as at_assign_f32, bit for bit, computed faster when most rows come with a correct
 * guess (a Lloyd iteration guessing the previous assignment).  Guesses are values in [0, k), or
 * anything else for "none", given either per row (hint_ids: int64 [n]) or per visiting position
 * (hint_sorted: uint32 [n], the guess of row order[p] at position p; needs order).  order_or_null:
 * uint32 [n], a permutation of the rows that groups equal guesses.  at_centroid_accum_f32 produces
 * both arrays for the ids it was given (order_out, sorted_ids_out).  ids must not alias hint_ids.
 * Results do not depend on the hints or the order. */
int at_assign_hinted_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k,
                         const int64_t* hint_ids_or_null, const uint32_t* order_or_null,
                         const uint32_t* hint_sorted_or_null, int64_t* ids, float* dist_or_null,
                         void* stream);

/* ---- exact pruning for Lloyd iterations (none of this changes any result) ----------------------
 * at_group_rows_kd_host: spatial grouping of the centroid table into groups of `leaf` rows (host
 *   arrays; perm_out: ceil(k/leaf)*leaf entries, -1 padded).
 * at_group_min_dist_f32: dmin[p][g] (DEVICE float [k][ng]) = a lower bound of the distance from
 *   centroid p to the nearest member of group g (groups of 32 as listed in cperm, DEVICE int32).
 * at_visit_order_f32: rows sorted by (previous id, previous distance): order_out and the ids in
 *   that order (both DEVICE uint32 [n]).
 * at_group_means_f32: means[g] (DEVICE float [ng][d]) = mean row of group g.
 * at_group_neighbours_f32: gnbr[g] (DEVICE uint32 [ng][ceil(ng/32)]) = bit set of the nnb groups whose
 *   means are nearest to mean g, g itself included (ng <= 512, d <= 128); input of the guess generators.
 * at_assign_pruned_f32 (arguments: struct at_pruned_args below).  guess_only = 0: the answer of at_assign_f32, bit
 *   for bit (d = 64 or 128, n >= 20, ng <= 512).  Every row's guess hint_sorted[p] (for row order[p]) is scored
 *   exactly first; a 32-centroid group is then skipped for a 32-row tile when the triangle inequality, with a margin
 *   that covers the fp32 rounding of the distances, rules it out for all of the tile's rows.
 *   guess_only = 1 (a guess generator, NOT exact): hint_sorted holds a GROUP id per row; each row gets the best
 *   centroid among the groups named by its 32-row tile; `bounds` is then read as an optional uint32
 *   [ng][ceil(ng/32)] table: bit set = group worth searching for a row naming g.  The unguided exact search is
 *   nearest group mean -> guess_only = 1 -> guess_only = 0 with those answers as guesses.
 *   use_filter != 0: stage 1 is the fp16-split filter (csrc/filter.hip: three fp16 MFMAs per fp32 one, a winner
 *   accepted only when the runner-up is provably out of reach of the fp32 contract), the remaining rows are redone in
 *   fp32: ids/dist are bit-identical to use_filter = 0, and the call needs no host round trip (the redo kernel reads
 *   the list length on the device) unless earlier calls on this context listed more than n/16 rows.
 *   image_current != 0: the caller vouches that the fp16 image at_group_min_dist_f32 built is still current (same c,
 *   cperm; centroids unchanged since), so it is reused. */
int at_group_rows_kd_host(const float* rows_host, int k, int d, int leaf, int32_t* perm_out_host);
int at_group_min_dist_f32(at_ctx* ctx, const float* c, int k, int d, const int32_t* cperm, int ng,
                          float* dmin, void* stream);
int at_visit_order_f32(at_ctx* ctx, const int64_t* ids, const float* dis_or_null, int64_t n, int k,
                       uint32_t* order_out, uint32_t* hint_sorted_out, void* stream);
int at_group_means_f32(at_ctx* ctx, const float* c, int k, int d, const int32_t* cperm, int ng,
                       float* means, void* stream);
int at_group_neighbours_f32(at_ctx* ctx, const float* means, int ng, int d, int nnb, uint32_t* gnbr,
                            void* stream);
typedef struct at_pruned_args {
    const float* x;              /* DEVICE [n][d] rows */
    int64_t n;
    int d;
    const float* c;              /* DEVICE [k][d] centroids */
    int k;
    const uint32_t* order;       /* DEVICE [n]: rows in visiting order (at_visit_order_f32) */
    const uint32_t* hint_sorted; /* DEVICE [n]: the guess of row order[p] (guess_only: its group) */
    const int32_t* cperm;        /* DEVICE [ng*32]: spatial grouping (at_group_rows_kd_host), -1 padded */
    int ng;
    const float* bounds;         /* DEVICE: dmin [k][ng] (at_group_min_dist_f32); guess_only: optional bit table */
    int guess_only;              /* 0 = exact search, 1 = guess generator */
    int use_filter;              /* 0 = fp32 pruned sweep, 1 = fp16-split filter first (same bits) */
    int prepass_done;            /* 1 = at_prune_mask_f32 ran just before with the same arguments */
    int image_current;           /* 1 = the fp16 image of (c, cperm) left by at_group_min_dist_f32 is still valid */
    int64_t* ids;                /* DEVICE [n] out */
    float* dist_or_null;         /* DEVICE [n] out */
} at_pruned_args;
int at_assign_pruned_f32(at_ctx* ctx, const at_pruned_args* args, void* stream);
/* The pre-pass of at_assign_pruned_f32 alone (per-row bound and per-tile group masks into the
 * context's workspace).  at_assign_pruned_f32 runs it itself unless prepass_done != 0, in which case
 * it must directly follow this call with the same arguments on the same stream. */
int at_prune_mask_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k,
                      const uint32_t* order, const uint32_t* hint_sorted, int ng,
                      const float* dmin_or_null, int mode, void* stream);

/* (Counters of the pruned / filtered sweeps and the stage-1 test hook live in at_debug.h.) */
/* Guess generator for rows in their own (coherent) order -- consecutive frames of clips, i.e. tokenise:
 * nearest of the ng group means (means [ng, d], at_group_means_f32) -> the groups the neighbour table
 * gnbr [ng][ceil(ng/32)] names -> best centroid among them, one launch, rows read once.  ids are guesses
 * for at_visit_order_f32 / at_assign_pruned_f32; dist (may be NULL) approximate distances. */
int at_assign_coarse_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k,
                         const int32_t* cperm, int ng, const float* means, const uint32_t* gnbr,
                         int64_t* ids, float* dist, void* stream);


/* The same m entries as at_rand_perm_prefix_mt19937(n, seed, m, .), bit for bit, computed on the device
 * (csrc/randperm.hip: the mt19937 stream by one workgroup, then the Fisher-Yates prefix resolved with a
 * sort of the swap partners instead of 2 M dependent host cache misses).  prefix: DEVICE int32 [m].  Uses
 * workspace of its own, so it may run on a stream beside other calls on the same context. */
int at_rand_perm_prefix_device(at_ctx* ctx, int64_t n, int64_t seed, int64_t m, int32_t* prefix, void* stream);

/* out[i] = x[idx[i]] (rows of d floats).  idx: DEVICE int32 [m]. */
int at_gather_rows_f32(at_ctx* ctx, const float* x, int d, const int32_t* idx, int64_t m,
                       float* out, void* stream);

/* faiss compute_centroids, accumulation half: sums[c] = sum of x[i] with ids[i] == c taken in
 * ASCENDING i with fp32 adds (bitwise what a single FAISS thread produces), counts[c] = number of
 * members (exact in fp32).  sums [k][d], counts [k] are overwritten.  order_out_or_null: uint32 [n],
 * receives the rows sorted by (id, row) -- the member lists, back to back; sorted_ids_out_or_null:
 * uint32 [n], the id of each of those rows (k for an id outside [0, k)). */
int at_centroid_accum_f32(at_ctx* ctx, const float* x, int64_t n, int d, const int64_t* ids, int k,
                          float* sums, float* counts, uint32_t* order_out_or_null,
                          uint32_t* sorted_ids_out_or_null, void* stream);

/* The same with a weight per row (faiss.Kmeans.train(x, weights=w); the single-rounding form is this library's
 * contract): for the members i0 < i1 < ... of cluster c in ASCENDING i,
 *     sums[c][f] = the chain s <- fmaf(x[i][f], w[i], s) from +0 (one rounding per member),
 *     wsums[c]   = the chain s <- s + w[i] from +0, in the same order.
 * With every weight 1.0f both are the bits of at_centroid_accum_f32.  w: DEVICE float [n]; nothing about its values is
 * checked (NaN, Inf and negative weights follow the formula).  sums [k][d], wsums [k] are overwritten; ids outside
 * [0, k) are parked; order_out_or_null / sorted_ids_out_or_null as above.  Everything is queued on `stream` (no side
 * stream, nothing to join); the call uses workspace slots of its own, so it may run beside at_centroid_accum_f32 on
 * another stream of the same context, and a weighted call on another stream than the previous one waits for it. */
int at_centroid_accum_weighted_f32(at_ctx* ctx, const float* x, const float* w, int64_t n, int d, const int64_t* ids,
                                   int k, float* sums, float* wsums, uint32_t* order_out_or_null,
                                   uint32_t* sorted_ids_out_or_null, void* stream);

/* faiss compute_centroids, scaling half, over n_parts partial results (p = data-parallel rank):
 * part p has its sums [k][d] at sums_parts + p*sums_part_stride and its counts [k] at
 * counts_parts + p*counts_part_stride (strides in floats).  Partials are added in ascending p,
 * then centroids[c] = sum * (1/count) where count > 0 and 0 where the cluster is empty;
 * hassign[c] = count. */
/* Long member lists are accumulated on a side stream of the context.  By default at_centroid_accum_f32
 * makes `stream` wait for it before returning; after at_centroid_accum_defer(ctx, 1) that wait is left to
 * at_centroid_accum_join(ctx, stream), which must precede any use of sums / counts -- work queued on
 * `stream` in between overlaps the long lists. */
int at_centroid_accum_defer(at_ctx* ctx, int on);
int at_centroid_accum_join(at_ctx* ctx, void* stream);

int at_centroid_finalize_f32(at_ctx* ctx, const float* sums_parts, int64_t sums_part_stride,
                             const float* counts_parts, int64_t counts_part_stride, int n_parts,
                             int k, int d, float* centroids, float* hassign, void* stream);

/* out[i] = parts[0][i] + parts[1][i] + ... added in ascending part order (part p at parts + p*part_stride floats, m
 * floats each): the fixed-order reduction of the data-parallel exchange when it runs as all-to-all + local sum +
 * all-gather instead of an all-gather of whole partials (same bits as at_centroid_finalize_f32 over all parts). */
int at_sum_parts_f32(at_ctx* ctx, const float* parts, int64_t part_stride, int n_parts, int64_t m, float* out,
                     void* stream);

/* The exchange itself, for hosts that do not go through torch.distributed (the Python layer does: ops._Dist):
 * thin wrappers over RCCL on the CALLER's communicator (`nccl_comm` is an ncclComm_t; RCCL is looked up at run time,
 * the library has no link-time dependency on it).  at_comm_allgather_f32: parts [n_ranks][count] <- every rank's
 * part [count].  at_comm_allreduce_ordered_f32: out [count] <- the parts added in ascending rank order (all-gather into
 * parts_scratch [n_ranks * count], then at_sum_parts_f32): the all-reduce of the sharded Lloyd iteration, the same
 * bits on every rank and in the oracle's n_shards mode -- which ncclAllReduce(sum) does not promise. */
int at_comm_allgather_f32(at_ctx* ctx, void* nccl_comm, const float* part, float* parts, int64_t count, void* stream);
int at_comm_allreduce_ordered_f32(at_ctx* ctx, void* nccl_comm, const float* part, float* parts_scratch, float* out,
                                  int64_t count, void* stream);

/* at_split_clusters_host on DEVICE buffers (hassign [k], centroids [k][d], both updated in place), same bits:
 * one workgroup regenerates the mt19937(1234) stream in LDS and runs the cyclic acceptance scans, so a Lloyd
 * iteration needs no host round trip to learn whether a cluster came out empty.  *nsplit_out (DEVICE int32)
 * receives the number of re-seeded clusters (-1: no donor exists, i.e. every cluster has at most one member). */
int at_split_clusters_f32(at_ctx* ctx, int d, int k, int64_t n, float* hassign, float* centroids,
                          int32_t* nsplit_out, void* stream);

/* Statistics of one Lloyd iteration, left on the device (faiss ClusteringIterationStats): stats[0] = objective =
 * the doubles obj_parts[p * obj_part_stride], p < n_parts, added in ascending p (one per data-parallel rank: its
 * at_sum_f32 of the distances); stats[1] = imbalance factor k * sum(h^2) / (sum h)^2 of hassign [k]. */
int at_lloyd_stats_f64(at_ctx* ctx, const float* hassign, int k, const double* obj_parts,
                       int64_t obj_part_stride, int n_parts, double* stats, void* stream);

/* at_lloyd_stats_f64 followed by at_split_clusters_f32 in ONE launch (both are single-workgroup kernels over the k
 * counts; a Lloyd iteration of a sharded run is short enough for the launch between them to matter).  stats may be
 * null: then exactly at_split_clusters_f32. */
int at_lloyd_stats_split_f32(at_ctx* ctx, int d, int k, int64_t n, float* hassign, float* centroids, int32_t* nsplit_out,
                             const double* obj_parts, int64_t obj_part_stride, int n_parts, double* stats, void* stream);

/* *out (DEVICE double) = sum of v[0..n) accumulated in double with a fixed reduction tree. */
int at_sum_f32(at_ctx* ctx, const float* v, int64_t n, double* out, void* stream);

/* 1 if any of v[0..n) is NaN/Inf else 0, written to *flag (DEVICE int32). */
int at_any_nonfinite_f32(at_ctx* ctx, const float* v, int64_t n, int32_t* flag, void* stream);

/* The same verdict for the unit rows at_logmel_f32(..., fuse_l2norm = 1) has written since the last call, without
 * reading them again: the unit-row pass sets a flag in the context when a row's squared norm is not finite (a NaN or
 * Inf in the row; also squares that overflow, so a caller confirms a raised flag with at_any_nonfinite_f32).  Writes
 * 0 / 1 to *flag (DEVICE int32) and clears the context's flag, in stream order.  Replaces the scan faiss makes of
 * its training input (Clustering::train: FAISS_THROW_IF_NOT_MSG(std::isfinite(x_in[i]), ...), reached from
 * processors/cluster_creator.py:54-56) on the path where this library produced that input itself. */
int at_logmel_nonfinite_take(at_ctx* ctx, int32_t* flag, void* stream);

/* counts[t] = number of i with ids[i] == t, t in [0, k) (ids outside are skipped): the token statistics of
 * processors/spec_tokenizer.py:129-147 (a Python Counter over tokens.tolist()) without leaving the device. */
int at_token_histogram_i64(at_ctx* ctx, const int64_t* ids, int64_t n, int k, int64_t* counts, void* stream);

/* Rank-frequency statistics of that histogram, still on the device (processors/spec_tokenizer.py:146-240:
 * sorted(Counter.items()), np.cumsum / np.searchsorted, scipy.stats.linregress on the log-log curve).
 *   sorted_counts[r], sorted_tokens[r] (DEVICE int64 / int32 [k]): the r-th most frequent token and its count
 *     (ties in ascending token id; tokens that never occur come last with count 0);
 *   stats (DEVICE double [8]): [0] total occurrences; [1] U = tokens that occur; [2] the number of ranks whose
 *     cumulative share of the occurrences is below 0.8 (np.searchsorted(cumsum / total, 0.8)); [3] slope,
 *     [4] intercept, [5] r of the least-squares line through (ln rank, ln count) over the ranks
 *     [int(0.1 U), int(0.9 U)) (linregress' formulas, double); [6] the number of points of that fit. */
int at_token_stats_f64(at_ctx* ctx, const int64_t* counts, int k, int64_t* sorted_counts,
                       int32_t* sorted_tokens, double* stats, void* stream);

/* Exact silhouette of a labelled sample: sklearn.metrics.silhouette_samples / silhouette_score on float32 rows, the
 * metric ClusterCreator.evaluate_clustering reports (processors/cluster_creator.py:115-117:
 * silhouette_score(data, labels, sample_size=10000)).  x: DEVICE [n][d] fp32 rows; labels: DEVICE int64 [n], any
 * values (only those present count, as after sklearn's LabelEncoder).  sklearn's float32 recipe, in fp64:
 *   d2 = fl32(((-2 <x_i,x_j>) + |x_i|^2) + |x_j|^2) (dot and norms in fp64), max(d2, 0), 0 for i == j,
 *   dist = correctly rounded fp32 sqrt;  S[i,c] = fl32(fp64 sum of dist(i,j) over the members j of c, j ascending);
 *   a = fl32(S[i,own] / (n_own - 1)), b = min over c != own of fl32(S[i,c] / n_c);
 *   s[i] = fl32(fl32(b - a) / max(a, b)), NaN -> 0 (singleton clusters, a = b = 0).
 * s: DEVICE fp32 [n] in the caller's row order; *sum (DEVICE double) = fp64 sum of s (score = *sum / n);
 * *n_labels (DEVICE int64) = number of distinct labels.  sklearn requires 2 <= n_labels <= n - 1: outside that
 * range s and *sum are computed but meaningless, and checking is the caller's.  Rows must be finite (the caller's
 * check, as sklearn's check_array).  Deterministic: two calls give the same bits.  n < 2^31. */
int at_silhouette_f32(at_ctx* ctx, const float* x, int d, const int64_t* labels, int64_t n, float* s,
                      double* sum, int64_t* n_labels, void* stream);

/* Exact per-class average precision and its mean over the classes with a positive: what
 * MetricsCalculator.compute_metrics reports as mAP after every epoch (utils/metrics_calculator.py:8-33, called from
 * processors/model_trainer.py:96: sklearn.metrics.average_precision_score per class, np.mean over the classes whose
 * labels sum to more than 0).  scores, labels: DEVICE fp32, sample-major [n][c] with row strides ld_scores,
 * ld_labels >= c (in floats); labels are 0.0 or 1.0.  Per class, sklearn's recipe: sort by score descending, equal
 * scores (-0.0 == +0.0) form one group, and over the groups g in that order
 *   ap[j] = sum_g fl(fl((tp_g - tp_{g-1}) / P) * fl(tp_g / cnt_g))      fp64; tp_g, cnt_g, P exact integers
 * (tp_g / cnt_g: positives / samples up to the end of g; P = n_pos[j]); groups without a positive add nothing, the
 * others are added in one fixed order, so |ap[j] - AP| <= 2 (P + 2) 2^-53.  NaN where n_pos[j] == 0.
 *   ap: DEVICE double [c]; n_pos: DEVICE int64 [c];
 *   map: DEVICE double [2]: the rounded sum of ap over the classes with positives (ascending class order) and their
 *     number -- mAP = map[0] / map[1], or the reference's 0.0 when map[1] == 0;
 *   flags: DEVICE int32: bit 0 = a score is NaN or infinite (sklearn raises ValueError), bit 1 = a label is neither 0.0
 *     nor 1.0.  With a flag set the other outputs are meaningless.
 * Deterministic, and the same bits for every chunking of the classes (the two sort buffers of a chunk stay within 1 GiB
 * of context workspace unless a single class needs more); no host synchronisation once the workspace has its size.
 * 1 <= n < 2^31 (and 16 n bytes of workspace for the keys of one class), c >= 1.  A call on another stream than the
 * context's previous at_average_precision_f32 waits for that call. */
int at_average_precision_f32(at_ctx* ctx, const float* scores, int64_t ld_scores, const float* labels, int64_t ld_labels,
                             int64_t n, int c, double* ap, int64_t* n_pos, double* map, int32_t* flags, void* stream);

/* Exact per-class ROC AUC and its mean, and with ap / map non-NULL the average precision of at_average_precision_f32 (the
 * same bits for every chunking) from the same sort: mAP, mAUC and d' are the triple AudioSet results are reported in.
 * Inputs, strides, limits, flags, chunking and workspace are at_average_precision_f32's (the two entries share the
 * context's workspace: a call on another stream than the previous call of either waits for it).  Per class, with the
 * groups g of equal scores in descending order (-0.0 == +0.0), tp_g / fp_g the positives / negatives up to the end of g,
 * P = n_pos[j] and N = n - P:
 *   two_u[j] = sum_g (fp_g - fp_{g-1}) (tp_g + tp_{g-1})       an exact integer, <= 2 P N < 2^61
 *   auc[j]   = (double)two_u[j] / (double)(2 P N)              NaN when P == 0 or N == 0
 * sklearn's roc_auc_score (the trapezoid rule over roc_curve) in exact arithmetic: the correctly rounded quotient of two
 * correctly rounded integers, so |auc - AUC| <= 3 * 2^-53 (+ O(2^-106)), and sklearn's own value lies within
 * (G + 10) 2^-53 of auc, G the number of groups.
 *   ap: DEVICE double [c] or NULL; map: DEVICE double [2] or NULL (both or neither);
 *   auc: DEVICE double [c]; two_u, n_pos: DEVICE int64 [c];
 *   mauc: DEVICE double [2]: the rounded sum of auc over the classes with a positive and a negative (ascending class
 *     order) and their number -- mAUC = mauc[0] / mauc[1]. */
int at_ranking_metrics_f32(at_ctx* ctx, const float* scores, int64_t ld_scores, const float* labels, int64_t ld_labels,
                           int64_t n, int c, double* ap, double* map, double* auc, int64_t* two_u, int64_t* n_pos,
                           double* mauc, int32_t* flags, void* stream);

/* The counts behind the reference's threshold metrics (utils/metrics_calculator.py:13-21: f1_score micro / macro and
 * hamming_loss on predictions > config.prediction_threshold).  predicted = score > threshold, strict and in fp32 (what
 * numpy's comparison of a float32 array with a Python float does; -0.0 == +0.0).  scores, labels, strides and flags as
 * for at_average_precision_f32; 1 <= n < 2^31, 1 <= c <= 32768; threshold finite.
 *   counts: DEVICE int64 [c][3]: per class tp (predicted, label 1), fp (predicted, label 0), fn (not predicted, label 1).
 * Integers: deterministic.  No workspace, no host synchronisation. */
int at_threshold_counts_f32(at_ctx* ctx, const float* scores, int64_t ld_scores, const float* labels, int64_t ld_labels,
                            int64_t n, int c, float threshold, int64_t* counts, int32_t* flags, void* stream);

/* The k nearest centroids under squared L2 (IndexFlatL2.search(x, k)).  dis(i,j) is at_assign_f32's value bit for bit
 * (the direct form for n < 20); a centroid is listed only if dis(i,j) < +inf (NaN never is).  Row i of the output holds
 * the k smallest (dis, j) in lexicographic order, ascending (ties: lower j first); slots with nothing to list hold
 * id -1 and +inf (k > k_c, NaN rows, rows whose distances all overflow).  So ids[i*k] / dist[i*k] equal
 * at_assign_f32's answer for every finite row.
 *   x: [n][d] fp32; c: [k_c][d] fp32, 1 <= k_c <= 2^24; k >= 1 (k < 1: AT_E_INVALID);
 *   ids: int64 [n][k]; dist_or_null: float [n][k].
 * 2 <= k <= 32 on 16-byte aligned rows with d % 4 == 0 and n >= 20: one fused sweep with a running top-k per row.
 * Otherwise blocks of rows x all centroids of sort keys (at most 256 MiB of context workspace) and a segmented radix
 * sort per row.  A call on another stream than the context's previous at_knn_f32 waits for that call. */
int at_knn_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k_c, int k, int64_t* ids,
               float* dist_or_null, void* stream);

/* The centroid with the largest inner product (IndexFlatIP.search(x, 1); the search of spherical k-means).
 *   ip(i,j) = fmaf chain over the feature index, ascending, from +0 (v_mfma_f32_32x32x2_f32): the ip of at_assign_f32,
 *   at every n (faiss's small-batch form is the same sum).  Centroid j is listed for row i iff ip(i,j) > -inf: a NaN
 *   product never is, +inf is.  ids[i] = the lowest j among the listed centroids with the largest ip(i,j); ip[i] = that
 *   product with its own bits.  Rows with nothing to list (NaN rows) get ids = -1, ip = -inf (faiss's heap would leave
 *   -FLT_MAX there).  A product of zero keeps the sign the chain gives it, at every d: a negative term that underflows
 *   rounds to -0, and -0 and +0 compare equal, so the sign never decides an id.
 *   x: [n][d] fp32; c: [k][d] fp32, 1 <= k <= 2^24; ids: int64 [n]; ip_or_null: float [n].  n == 0 is a no-op.
 * d % 4 == 0 on 16-byte aligned rows: one dense MFMA sweep (x in registers at d = 64 and 128, re-read per 64-feature
 * chunk otherwise); everything else: the same chain in scalar code.  Like at_assign_f32 the call keeps its centroid
 * image in the context: calls of one context are ordered by their streams. */
int at_assign_ip_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k, int64_t* ids,
                     float* ip_or_null, void* stream);

/* faiss fvec_renorm_L2 on every row of c [k][d], in place (spherical k-means: the centroids after every update).
 *   nr = fmaf chain of c[f] * c[f], ascending, from +0.  nr > 0: inv = 1.0f / sqrtf(nr), both correctly rounded, and
 *   c[f] = c[f] * inv, one rounding each (faiss divides in double and narrows: the same value).  Otherwise (a zero row, a
 *   row that holds a NaN) the row is left untouched.  An nr that overflows gives inv = 0.  One launch. */
int at_renorm_rows_f32(at_ctx* ctx, float* c, int64_t k, int d, void* stream);

/* Product quantiser, encoder (faiss ProductQuantizer::compute_codes at nbits = 8).  A row of d features is cut into M
 * sub-vectors of dsub = d / M features; sub-space m has the codebook codebooks[m] of ksub rows.  codes[i][m] is
 * at_assign_f32's answer for (sub-vector m of the rows as an [n][dsub] matrix, codebooks[m]), bit for bit: ascending fmaf
 * chains for |x|^2, |c|^2 and <x, c> over the dsub features, dis = fma(-2, ip, xn + cn), the clamp v < 0 ? 0 : v, the
 * lowest index on equal distances, and the direct form sum (x-c)^2 when the CALL has n < 20 rows.  A sub-vector with no
 * distance below +inf (a NaN or Inf in it, or overflow) gets code 0 and distance +inf, and sets *bad.
 *   x: [n][d] fp32; codebooks: [M][ksub][d/M] fp32; 1 <= ksub <= 256, d % M == 0, n >= 0 (n == 0 is a no-op that
 *   touches no pointer); codes: uint8 [n][M]; dist_or_null: float [n][M], the winning distances; bad_or_null: DEVICE
 *   int32, written by every call with n > 0: 0, then 1 if some sub-vector had nothing to list.
 * ksub == 256, dsub % 4 == 0, 16-byte aligned rows, n >= 20 and d + M <= 160 (all M codebooks and their norms in the
 * 160 KiB of LDS of a CU): one launch in which every workgroup keeps the whole MFMA-operand image of the codebooks in
 * LDS and x is read once.  Everything else: one thread per (row, sub-space) with the same chains in scalar code.  The
 * fused form keeps its image in the context: a call on another stream than the context's previous one waits for it. */
int at_pq_encode_f32(at_ctx* ctx, const float* x, int64_t n, int d, int M, int ksub, const float* codebooks,
                     uint8_t* codes, float* dist_or_null, int32_t* bad_or_null, void* stream);

/* Product quantiser, decoder: out[i][m * dsub + f] = codebooks[m][codes[i][m]][f], copied bits (a code >= ksub, which
 * no encoder produces, decodes to NaN).  Sizes as for at_pq_encode_f32; out: float [n][d].  16-byte accesses where
 * dsub % 4 == 0 and codebooks / out are 16-byte aligned, one float per thread otherwise.  No workspace. */
int at_pq_decode_f32(at_ctx* ctx, const uint8_t* codes, int64_t n, int d, int M, int ksub, const float* codebooks,
                     float* out, void* stream);

/* Product quantiser, asymmetric-distance search over stored codes (faiss IndexPQ::search in its default ST_PQ mode,
 * recalled, NOT verified against faiss output: the contract is the library's own).  Query row x[i] gets the table
 *   T[i][m][j] = sum_f (x[i][m * dsub + f] - codebooks[m][j][f])^2, df = x - c one fp32 subtraction, acc = fmaf(df, df,
 *   acc) from +0 over f ascending -- the direct form whatever n is (at_assign_f32's arithmetic for calls of n < 20 rows);
 * database row r the distance dis(i, r) = T[i][0][codes[r][0]] + T[i][1][codes[r][1]] + ..., one fp32 addition per
 * step in ascending m, starting from the m = 0 entry.  Row r is listed for query i only if dis(i, r) < +inf (a NaN never
 * is); row i of the result holds the k smallest (dis, r), lexicographic and ascending, the lower id first on equal
 * distances; the places left over (ntotal < k, a NaN or Inf in the query, overflow) hold ids = -1, dist = +inf:
 * at_knn_f32's conventions.  No flag word: a non-finite query is not an error.  A stored code >= ksub (possible only
 * with ksub < 256) makes that database row unlisted for every query and is never used as an index.
 *   x: [n][d] fp32; codebooks: [M][ksub][d/M] fp32; codes: uint8 [ntotal][M]; d % M == 0, 1 <= M <= 64, 1 <= ksub <= 256,
 *   1 <= k <= 128, 0 <= ntotal < 2^31, n >= 0 (n == 0 is a no-op that touches no pointer; ntotal == 0 fills the outputs
 *   and does not touch codes); ids: int64 [n][k]; dist_or_null: float [n][k].  Anything else is AT_E_INVALID: there is
 *   no general path behind M <= 64 (the tables of a workgroup's queries stay in LDS) or k <= 128 (so do its candidates).
 * Two launches per chunk of queries (csrc/pq_search.hip): the scan -- a workgroup builds the tables of 4 queries (2 for
 * M > 32) in LDS, streams a slab of 65 536 code rows once with 16-, 8-, 4- or 1-byte loads as M and the pointer allow,
 * and keeps the k smallest keys per query -- and the merge of the slabs' lists.  No [n][ntotal] matrix exists anywhere;
 * the lists (8 bytes per query, slab and place) live in the context, a chunk of queries within 256 MiB (and 2^24 - 4 queries).  No host
 * synchronisation, no device-to-host copy; a call on another stream than the context's previous at_pq_search_f32 waits
 * for it. */
int at_pq_search_f32(at_ctx* ctx, const float* x, int64_t n, int d, int M, int ksub, const float* codebooks,
                     const uint8_t* codes, int64_t ntotal, int k, int64_t* ids, float* dist_or_null, void* stream);

/* Inverted lists over exact fp32 rows (faiss IndexIVFFlat under L2; ops.IndexIVFFlat; the contract is the library's
 * own).  The stored rows are kept grouped by list number, and a query is compared only with the rows of the lists it
 * probes.
 *   Probed lists: the entries of row i of probes ([n][nprobe] int64) that lie in [0, nlist); anything else (-1) is no
 *     list.  The entries of a row must be distinct -- ops passes row i of at_knn_f32(x, centroids, min(nprobe, nlist)),
 *     its direct form for n < 20 included; only the SET matters.
 *   Distance: dis(i, r) between query i and stored row r is ALWAYS the expansion form of at_assign_f32, whatever n is:
 *     ip, |x|^2, |r|^2 ascending fmaf chains, (xn + rn) - 2*ip in one fma, the clamp v < 0 ? 0 : v, which leaves a NaN a
 *     NaN.  Features padded with +0 (queries up to a multiple of 4, both sides up to the chunk of 64) change no bit.
 *   Result: row i lists the k smallest (dis, id) in lexicographic order over the stored rows of its probed lists with
 *     dis < +inf; the places left over hold ids = -1, dist = +inf.
 *   Consequence: with every list probed, n >= 20 and no stored row outside the lists, the result is at_knn_f32's over
 *     the stored rows, bit for bit.
 *
 * at_ivf_build_f32 makes the searchable image of rows [ntotal][d] (any d >= 1) whose list numbers are lists [ntotal]
 * int64 (outside [0, nlist): in no list, never found).  order [ntotal] int64 names the rows sorted by list number,
 * STABLY, so that ids ascend inside a list, with the rows of no list last (a position whose row is not of the list the
 * position belongs to becomes a pad: a wrong order loses rows, it cannot address out of range).  Outputs, all sized by
 * the caller from ntiles >= ntotal / 128 + nlist (a host-side bound: nothing is read back):
 *   img: float [ntiles][cs::tile_floats(4, ceil(d / 64))], csrc/chunked_sweep.h's chunked image, every list padded to
 *     whole tiles of 128 rows, a pad row all +0 with norm +inf; 16-byte aligned;
 *   pos2id: int32 [ntiles * 128], the id of the row at a position of the image, -1 for a pad;
 *   first: int32 [nlist + 1], the first tile of every list; first[nlist] = tiles in use.
 * 0 <= ntotal < 2^31, ntiles * 128 < 2^31, 1 <= nlist <= 2^24.  Three launches; the list counts live in the context.
 *
 * at_ivf_search_f32: x [n][d] fp32 with d % 4 == 0, 16-byte aligned -- d is the row width of the build rounded up to a
 * multiple of 4, the features behind the build's d being +0; img / ntiles / pos2id / first / ntotal / nlist as built;
 * 1 <= k <= 32 (the per-lane list of at_knn_f32's fused path; there is no path behind it), nprobe >= 1; ids: int64
 * [n][k]; dist_or_null: float [n][k].  n == 0 is a no-op that touches no pointer.  Anything else is AT_E_INVALID, before
 * any launch.  Per chunk of queries (their partial lists, 8 bytes per (query, probe, place), within 256 MiB of context
 * workspace): a counting sort of the (query, probe) pairs by list, the scan -- a workgroup of four waves takes one
 * (list, block of up to 128 probing queries), gathers the queries as the MFMA B operand, streams the list's tiles
 * through LDS by LDS-DMA and keeps at_knn_f32's running per-lane top-k; d = 64 and 128 keep the query in registers,
 * any other d re-reads it per chunk -- and the merge of a query's nprobe partial lists.  No host synchronisation, no
 * device-to-host copy; a call on another stream than the context's previous at_ivf_* call waits for it. */
int at_ivf_build_f32(at_ctx* ctx, const float* rows, const int64_t* lists, const int64_t* order, int64_t ntotal, int d,
                     int nlist, int ntiles, float* img, int32_t* pos2id, int32_t* first, void* stream);
int at_ivf_search_f32(at_ctx* ctx, const float* x, int64_t n, int d, const int64_t* probes, int nprobe, int nlist,
                      const float* img, int ntiles, const int32_t* pos2id, const int32_t* first, int64_t ntotal, int k,
                      int64_t* ids, float* dist_or_null, void* stream);

/* Product-quantiser codes behind inverted lists (faiss IndexIVFPQ under L2; ops.IndexIVFPQ; the contract is the
 * library's own -- recalled, not verified against faiss output).  The stored rows are kept as M code bytes grouped by
 * list number, and a query meets only the codes of the lists it probes.
 *   Probed lists: as for at_ivf_search_f32 -- the entries of row i of probes ([n][nprobe] int64) in [0, nlist), distinct
 *     within a row; anything else (-1) is no list.
 *   Distance: for query i and probed list l the query vector is q = x[i] - centroids[l], one fp32 subtraction per
 *     feature (by_residual), or x[i] itself when centroids_or_null is NULL.  The table is T[m][j] = sum_f (q[m * dsub + f]
 *     - codebooks[m][j][f])^2 in at_pq_search_f32's direct form (df one subtraction, acc = fmaf(df, df, acc) from +0 over
 *     ascending f) and dis(i, r) = T[0][code[r][0]] + T[1][code[r][1]] + ..., one fp32 addition per step in ascending m,
 *     for the rows r of list l.  The expansion form appears nowhere; faiss's precomputed-table decomposition of the
 *     residual distance is a different arithmetic and is not implemented.
 *   Result: row i holds the k smallest (dis, id) in lexicographic order over the stored rows of its probed lists with
 *     dis < +inf (a NaN never is); the places left over hold ids = -1, dist = +inf.  No flag word: a non-finite query
 *     lists nothing.  A stored code >= ksub (possible only with ksub < 256) makes that row unlisted and is never used as
 *     an index.
 *   Consequence: without centroids, with every list probed and no stored row outside the lists, the result is
 *     at_pq_search_f32's over the same codebooks and codes, bit for bit, for every n.
 *
 * at_ivfpq_build groups codes (uint8 [ntotal][M], 1 <= M <= 64) by the list numbers lists [ntotal] int64 (outside
 * [0, nlist): in no list, never found).  order [ntotal] int64 names the rows sorted by list number, STABLY, so that ids
 * ascend inside a list, with the rows of no list last (a position whose row is not of the list the position belongs to
 * becomes a pad: a wrong order loses rows, it cannot address out of range).  Outputs, all sized by the caller from
 * ngroups >= ntotal / 16 + nlist (a host-side bound: nothing is read back):
 *   grouped: uint8 [ngroups * 16][M], every list padded to whole groups of 16 rows (a list then starts at a multiple
 *     of 16 bytes for any M), pads all 0;
 *   pos2id: int32 [ngroups * 16], the id of the row at a position, -1 for a pad;
 *   first: int32 [nlist + 1], the first group of every list; first[nlist] = groups in use.
 * 0 <= ntotal < 2^31, ngroups * 16 < 2^31, 1 <= nlist <= 2^24.  Three launches; the list counts live in the context.
 *
 * at_ivfpq_search_f32: x [n][d] fp32 (any 4-byte alignment), codebooks [M][ksub][d / M], centroids_or_null [nlist][d];
 * grouped / ngroups / pos2id / first / ntotal / nlist as built (grouped is read with 16-, 8- or 4-byte loads where M and
 * its address allow); d % M == 0, 1 <= M <= 64, 1 <= ksub <= 256, 1 <= k <= 128, nprobe >= 1; ids: int64 [n][k];
 * dist_or_null: float [n][k].  n == 0 is a no-op that touches no pointer.  Anything else is AT_E_INVALID, before any
 * launch: there is no path behind M <= 64 (the tables of a workgroup's pairs stay in LDS) or k <= 128 (so do its
 * candidates).  Per chunk of queries (their partial lists, 8 bytes per (query, probe, place), within 256 MiB of context
 * workspace; at most 2^30 pairs): at_ivf_search_f32's counting sort of the (query, probe) pairs by list, in blocks of 4
 * pairs (2 for M > 32); the scan -- one workgroup per (list, block of pairs) builds the tables of its pairs in LDS and
 * walks the list's rows with at_pq_search_f32's look-up loop and candidate buffer; a list of any length is walked by its
 * own workgroups alone, long lists are not split --; and at_pq_search_f32's streaming merge over a query's nprobe * k
 * keys.  No host synchronisation, no device-to-host copy; a call on another stream than the context's previous
 * at_ivfpq_* call waits for it. */
int at_ivfpq_build(at_ctx* ctx, const uint8_t* codes, const int64_t* lists, const int64_t* order, int64_t ntotal, int M,
                   int nlist, int ngroups, uint8_t* grouped, int32_t* pos2id, int32_t* first, void* stream);
int at_ivfpq_search_f32(at_ctx* ctx, const float* x, int64_t n, int d, const int64_t* probes, int nprobe, int nlist,
                        const float* centroids_or_null, int M, int ksub, const float* codebooks, const uint8_t* grouped,
                        int ngroups, const int32_t* pos2id, const int32_t* first, int64_t ntotal, int k, int64_t* ids,
                        float* dist_or_null, void* stream);

/* Residual quantiser (RVQ), greedy encoder: beam width 1, M dependent stages.  r_0 = x; for m = 0 .. M-1 in order,
 * (codes[i][m], dist[i][m]) is at_assign_f32's answer for the rows r_m against codebooks[m] ([ksub][d]), bit for bit:
 * ascending fmaf chains for |r|^2, |c|^2 and <r, c> over the d features, dis = fma(-2, ip, rn + cn), the clamp
 * v < 0 ? 0 : v, the lowest index on equal distances, and the direct form sum (r-c)^2 when the CALL has n < 20 rows.
 * A row with no distance below +inf at a stage (a NaN or Inf in it, or overflow) gets code 0 and distance +inf there,
 * and sets *bad.  Then r_{m+1}[i][f] = r_m[i][f] - codebooks[m][codes[i][m]][f], one fp32 subtraction (a flagged row
 * subtracts row 0 like any other; a NaN stays a NaN).  Column M-1 of dist is the squared reconstruction error in the
 * expansion form.  The contract is the library's own, not verified faiss output (faiss's ResidualQuantizer defaults
 * to a beam of 5: at_rq_beam_encode_f32 below).
 *   x: [n][d] fp32; codebooks: [M][ksub][d] fp32; 1 <= ksub <= 256, M >= 1, d >= 1, n >= 0 (n == 0 is a no-op that
 *   touches no pointer); codes: uint8 [n][M]; dist_or_null: float [n][M]; residual_or_null: float [n][d], r_M, must
 *   not overlap x; bad_or_null: DEVICE int32, written by every call with n > 0: 0, then 1 if some row had nothing to
 *   list at some stage.
 * d = 64 or 128, n >= 20 and 16-byte aligned x, codebooks and residual: one launch for all M stages, the residual in
 * registers, the codebooks streamed through LDS from a chunked image kept in the context.  Everything else: one launch
 * of the same chains in scalar code, a workgroup per 8 rows, the residual in the caller's buffer or in the context.  A
 * call on another stream than the context's previous at_rq_encode_f32 waits for that call. */
int at_rq_encode_f32(at_ctx* ctx, const float* x, int64_t n, int d, int M, int ksub, const float* codebooks,
                     uint8_t* codes, float* dist_or_null, float* residual_or_null, int32_t* bad_or_null, void* stream);

/* Residual quantiser, decoder: out[i] = codebooks[0][codes[i][0]], copied, then out[i] = out[i] + codebooks[m][codes[i][m]]
 * for m = 1 .. M-1 in ascending order, one fp32 addition each (a code >= ksub, which no encoder produces, makes the
 * whole row NaN).  Sizes as for at_rq_encode_f32; out: float [n][d].  16-byte accesses where d % 4 == 0 and codebooks /
 * out are 16-byte aligned, one float per thread otherwise.  No workspace. */
int at_rq_decode_f32(at_ctx* ctx, const uint8_t* codes, int64_t n, int d, int M, int ksub, const float* codebooks,
                     float* out, void* stream);

/* Residual quantiser, one stage of the beam search.  A row has b_in partial codes (beams), beam s with the residual
 * r_in[i][s].  (D, I) = at_knn_f32's answer for the n * b_in residuals as ONE [n * b_in][d] call against the codebook
 * with k = min(b_out, ksub), bit for bit -- so its direct form is chosen by n * b_in < 20.  The candidates of row i are
 * the (s, t) with I[i * b_in + s][t] >= 0; the new beams are the b_out smallest by (D, s, I), lexicographic and
 * ascending (equal distances: the lower parent slot, then the lower word; -0 equals +0), slot 0 the best:
 *   parent[i][s'] = s, code[i][s'] = I, dist[i][s'] = D, r_out[i][s'][f] = r_in[i][s][f] - codebook[I][f], one fp32
 *   subtraction.
 * A slot for which no candidate is left (only on rows with NaN, Inf or overflowing distances) follows every filled
 * slot, takes parent 0, code 0 and distance +inf, subtracts word 0 from parent 0's residual, and sets *bad.
 *   r_in: [n][b_in][d] fp32; codebook: [ksub][d] fp32; 1 <= ksub <= 256; 1 <= b_in, b_out <= 32, b_out <= b_in * ksub;
 *   n >= 0 (n == 0 is a no-op that touches no pointer); r_out: [n][b_out][d], must not overlap r_in; parent: int32
 *   [n][b_out]; code: uint8 [n][b_out]; dist: float [n][b_out]; bad_or_null: DEVICE int32, written by every call with
 *   n > 0: 0, then 1 if some slot was left unfilled.
 * One launch behind at_knn_f32's own: nothing is read back.  The select kernel gives a row to a half-wave and moves
 * 16 bytes per lane where d % 4 == 0 and r_in, r_out and codebook are 16-byte aligned, one float otherwise.  The lists
 * live in the context: a call on another stream than the context's previous at_rq_beam_* call waits for it. */
int at_rq_beam_step_f32(at_ctx* ctx, const float* r_in, int64_t n, int b_in, int d, const float* codebook, int ksub,
                        int b_out, float* r_out, int32_t* parent, uint8_t* code, float* dist, int32_t* bad_or_null,
                        void* stream);

/* Residual quantiser, beam-search encoder.  B_0 = 1, R_0[i][0] = x[i]; stage m = 0 .. M-1 is at_rq_beam_step_f32 with
 * b_in = B_m, b_out = B_{m+1} = min(beam, B_m * ksub) and codebooks[m].  codes[i][.] is the path of slot 0 behind the
 * last stage, dist[i][m] the distance at which that path's stage-m ancestor was chosen (column M-1: the final squared
 * error in the expansion form), residual[i] = R_M[i][0].  beam = 1 gives at_rq_encode_f32's three outputs bit for bit.
 * The contract is the library's own (faiss's beam search works from look-up tables of inner products, which changes
 * the arithmetic; it is not implemented).
 *   x, codebooks, codes, dist_or_null, residual_or_null, bad_or_null, n, d, M, ksub: as for at_rq_encode_f32;
 *   1 <= beam <= 32.  *bad is set when any slot of any stage was left unfilled.
 * Rows are taken in blocks whose workspace (two residual buffers, the lists of one stage, the records of all stages)
 * stays within 256 MiB; a block of a call with n >= 20 rows never has fewer than 20 (the distance form is the call's).
 * Per block and stage: at_knn_f32's launches and the select kernel; per block one back-trace kernel.  No host
 * synchronisation, no device-to-host copy.  A call on another stream than the context's previous at_rq_beam_* call
 * waits for it. */
int at_rq_beam_encode_f32(at_ctx* ctx, const float* x, int64_t n, int d, int M, int ksub, const float* codebooks,
                          int beam, uint8_t* codes, float* dist_or_null, float* residual_or_null, int32_t* bad_or_null,
                          void* stream);

/* ---- MFCC and delta features of log-mel rows (torchaudio.transforms.MFCC, ComputeDeltas; csrc/mfcc.hip) ----------
 * Input: log-mel rows x[g][n], frame-major [n_frames][n_mels] fp32, as at_logmel_f32 / at_logmel_ragged_f32 leave them,
 * and a DEVICE prefix first_frame[n_clips + 1] (int64, exclusive, non-decreasing, first_frame[0] = 0, last entry =
 * n_frames): clip i owns the frames [first_frame[i], first_frame[i + 1]); empty clips are allowed.
 *   top_db (use_top_db != 0): floor_i = (max over every value of clip i) - top_db, one fp32 subtraction; every value v
 *     of the clip becomes v < floor_i ? floor_i : v; a clip that holds a NaN becomes NaN throughout.  The maximum is per
 *     clip, always: amplitude_to_DB on a clip passed alone (torchaudio takes one maximum over a whole [B, L] batch).
 *   DCT table: dct[n][k], [n_mels][n_mfcc]; null = the table of at_dct_matrix_host(n_mfcc, n_mels, 1, .), built on the
 *     host and uploaded by the call.
 *   coefficients: c[g][k] = the fp32 fmaf chain over n = 0 .. n_mels - 1, ascending, from +0:
 *     acc = fmaf(x[g][n], dct[n][k], acc).
 *   deltas: win_length odd and >= 3, N = (win_length - 1) / 2; for frame t of a clip with T frames, acc = +0, then for
 *     j = 1 .. N ascending acc = fmaf((float)j, c[clamp(t + j)] - c[clamp(t - j)], acc), the difference one fp32
 *     subtraction, clamp to [0, T - 1] of the frame's own clip; delta[t] = acc / denom, one IEEE fp32 division, denom =
 *     (float)(N (N + 1) (2N + 1) / 3).  (compute_deltas with mode="replicate" in exact arithmetic; a constant clip and
 *     T = 1 give exactly +0.)  The second order is the same operator applied to the first.  orders: 0, 1 or 2.
 *   out: D = n_mfcc * (1 + orders) features per frame, feature o * n_mfcc + k.  AT_LAYOUT_FRAME_MAJOR: [n_frames][D];
 *     AT_LAYOUT_MEL_MAJOR (feature-major): clip i is a contiguous [D][T_i] block at D * first_frame[i] floats.
 *   A NaN or Inf frame gives NaN coefficients by the chain's own arithmetic and reaches at most orders * N frames on
 *   either side through the deltas, never another clip.  No flag is set by this call.
 * One launch (top_db: a memset and a small reduction launch in front of it, the per-clip maxima in a workspace slot of
 * the context: a call on another stream than the context's previous top_db call waits for it).  16-byte stores where
 * D % 4 == 0, the layout is frame-major and out is 16-byte aligned.  n_frames == 0 or n_clips == 0: nothing is launched.
 * Errors: null pointers, win_length even or < 3 (checked whatever `orders` is), orders outside 0..2, n_mfcc outside
 * [1, n_mels], n_mels outside the log-mel range, top_db < 0 (or NaN) when used, a window whose halo does not fit in LDS
 * beside n_mels-wide rows (win_length <= 9 fits at every width). */
int at_dct_matrix_host(int n_mfcc, int n_mels, int ortho, float* dct_host);
int at_mfcc_f32(at_ctx* ctx, const float* logmel, const int64_t* first_frame, int64_t n_clips, int64_t n_frames,
                int n_mels, int n_mfcc, const float* dct_or_null, int orders, int win_length, int use_top_db,
                float top_db, float* out, int layout, void* stream);
/* The delta operator alone: rows [n_frames][F] -> out [n_frames][F], delta[t] as above over the rows of each clip. */
int at_deltas_f32(at_ctx* ctx, const float* rows, const int64_t* first_frame, int64_t n_clips, int64_t n_frames, int F,
                  int win_length, float* out, void* stream);

/* ---- FLAC: torchaudio.load(path) for the reference's .flac files (processors/spectrogram_generator.py:99) --------
 * Native FLAC streams of 1-8 channels and 4-24 bits per sample.  The host finds the frames, the device decodes them:
 * one record per audio frame, every frame independent of the others. */
#define AT_E_FLAC_NOT_FLAC (-7)    /* no "fLaC" marker (behind an optional ID3v2 tag) */
#define AT_E_FLAC_UNSUPPORTED (-8) /* Ogg-encapsulated FLAC, bits per sample above 24 or below 4, STREAMINFO missing */
#define AT_E_FLAC_CORRUPT (-9)     /* metadata cut short, a frame chain that does not reach STREAMINFO's sample count */

/* status of a frame / a clip after at_flac_decode_f32 (a clip reports the kind of its first failing frame) */
#define AT_FLAC_OK 0
#define AT_FLAC_BAD_SUBFRAME 1 /* subframe header: padding bit set, reserved type, wasted bits >= sample width,
                                  predictor order above the block size */
#define AT_FLAC_RESERVED 2     /* reserved residual method, LPC precision 1111, negative LPC shift, a partition order
                                  the block size does not allow */
#define AT_FLAC_OVERRUN 3      /* the bit reader ran past the frame's bytes */
#define AT_FLAC_CRC16 4        /* frame CRC-16 mismatch */
#define AT_FLAC_BAD_RECORD 5   /* the frame record itself points outside the buffers it was given with */

typedef struct at_flac_info {
    int32_t channels, bits_per_sample, sample_rate;
    int32_t min_block, max_block;   /* STREAMINFO's block size range */
    int32_t variable_blocksize;     /* blocking strategy bit of the frames (0 when there are none) */
    int64_t total_samples;          /* per channel; the sum of the block sizes when STREAMINFO says 0 */
} at_flac_info;

typedef struct at_flac_frame {
    int64_t offset;        /* byte offset of the frame's sync code (indexer: in the file; decoder: in `data`) */
    int64_t first_sample;  /* index of the frame's first sample in its channel row */
    int64_t out_base;      /* decoder: float index in `out` of the clip's [C][L] block (indexer: 0) */
    int64_t out_stride;    /* decoder: the clip's row stride L in floats (indexer: total_samples) */
    int32_t length;        /* bytes up to the next frame or the end of the file: a bound, not the exact frame length */
    int32_t block_size;    /* samples per channel, 1..65535 */
    int32_t channel_assignment; /* 0-7: n+1 independent channels, 8 left/side, 9 side/right, 10 mid/side */
    int32_t bits_per_sample;
    int32_t header_bytes;  /* length of the frame header, CRC-8 included */
    int32_t channels;
    int32_t clip;          /* decoder: which clip_status entry this frame reports to (indexer: 0) */
    int32_t reserved;
} at_flac_frame;

/* Reads one file's bytes (HOST): skips a leading ID3v2 tag, requires "fLaC", walks the metadata blocks (STREAMINFO
 * read, all others ignored) and lists every audio frame without decoding it.  A frame is accepted where the sync
 * pattern is followed by a header without reserved codes, whose CRC-8 matches, whose channels / sample size / sample
 * rate agree with STREAMINFO, whose block size is within STREAMINFO's maximum, whose coded number continues the chain
 * (frame number = previous + 1, or sample number = previous + previous block size, from 0) and which lies at least
 * STREAMINFO's minimum frame size behind the previous one.  frames_host: capacity records, or NULL with capacity 0;
 * *n_frames receives the number of frames found, of which min(*n_frames, capacity) were written -- a caller whose
 * table was too small calls again.  Returns AT_OK, or AT_E_FLAC_* / AT_E_INVALID with a message in at_last_error(). */
int at_flac_index_host(const uint8_t* data_host, int64_t n_bytes, at_flac_info* info, at_flac_frame* frames_host,
                       int64_t capacity, int64_t* n_frames);

/* Decodes n_frames frames, one lane each, stream-ordered, on the current device; the caller owns every buffer.
 *   data: DEVICE bytes, the files of a batch back to back, 4-byte aligned, data_bytes long and followed by at least
 *     8 more readable bytes;  frames: DEVICE [n_frames], the files' tables concatenated in clip order with offset
 *     rebased to `data` and clip / out_base / out_stride / channels filled in (n_frames < 2^28);
 *   out: DEVICE float [out_floats]; clip c's [C][L] block, channel-major, starts at its out_base; each sample is
 *     sample / 2^(bps-1), exact.  A frame writes only [first_sample, first_sample + block_size) of its rows;
 *   frame_status: DEVICE int32 [n_frames]; clip_status: DEVICE int32 [n_clips] -- AT_FLAC_*, 0 = every frame decoded
 *     and its CRC-16 matched.  The samples of a failed frame are unspecified.
 * Covers constant / verbatim / fixed 0-4 / LPC 1-32 subframes, wasted bits, both Rice methods, every partition
 * order, escaped partitions, the three stereo decorrelations; LPC sums are 64-bit.  Every loop is bounded by the
 * record (which is itself checked against data_bytes and out_floats) and no byte outside the 4-byte words that
 * overlap [offset, offset + length + 4) is read: a malformed frame ends in a status, not in a fault. */
int at_flac_decode_f32(const uint8_t* data, int64_t data_bytes, const at_flac_frame* frames, int64_t n_frames,
                       int32_t n_clips, float* out, int64_t out_floats, int32_t* frame_status, int32_t* clip_status,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AUDIO_TOKENS_AMD_H */
