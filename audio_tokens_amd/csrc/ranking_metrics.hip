// ranking_metrics.hip -- exact per-class ROC AUC beside the average precision, and the counts behind F1 / Hamming loss.
//
// Reference call sites: utils/metrics_calculator.py:13-21 (f1_score micro / macro and hamming_loss on
// predictions > config.prediction_threshold) and the AudioSet triple mAP / mAUC / d' that the reference's data set is
// reported in.
//
// ROC AUC.  For one class, sorted by score descending and cut into groups g of equal scores (-0.0 == +0.0; the keys, the
// sort and the tile records are ap_stages.h's, shared with at_average_precision_f32), with tp_g, fp_g the positives and
// negatives up to the end of g, P and N = n - P all of them:
//   two_u = sum_g (fp_g - fp_{g-1}) (tp_g + tp_{g-1})       auc = (double)two_u / (double)(2 P N)
// which is sklearn's roc_auc_score (the trapezoid rule over roc_curve) in exact arithmetic: two_u <= 2 P N < 2^61 is an
// integer, so its parts are added in any order (one 64-bit integer atomic per workgroup), and auc is the correctly
// rounded quotient of two correctly rounded conversions whatever the chunking.
// auc_terms_kernel, per (class, tile of 2048 positions): tp in front of the tile from the tile records; one segmented
// block scan carries (positions << 32 | positives) of the current group, seeded for the group that straddles the tile's
// start by walking the earlier tiles' tail records backwards; the thread that holds a group's LAST position adds
// (len_g - pos_g) (2 tp_g - pos_g).  auc_finish_kernel divides.
//
// Threshold counts.  tc_count_kernel reads the [n][c] block as it lies (coalesced rows, ap_pack_kernel's walk), keeps
// tp / fp / fn of a chunk of classes in LDS and adds them to the 64-bit counters at the end of the workgroup's rows.
#include "ap_stages.h"

namespace {

// ---- ROC AUC -------------------------------------------------------------------------------------------------
// the segmented sum of ap_seg over 64-bit values: positions of the group so far << 32 | its positives (both < 2^31)
struct auc_seg { uint32_t flag; uint64_t value; };
constexpr uint64_t AUC_ONE = (uint64_t)1 << 32;

__device__ __forceinline__ auc_seg auc_seg_combine(auc_seg a, auc_seg b) {
    auc_seg r;
    r.flag = a.flag | b.flag;
    r.value = b.flag ? b.value : a.value + b.value;
    return r;
}

// exclusive scan over the workgroup in thread order: the state in front of the thread's span
__device__ __forceinline__ auc_seg auc_block_exscan_seg(auc_seg v, auc_seg* lds /*[WG / 64]*/) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        auc_seg o;
        o.flag = __shfl_up(v.flag, d, 64);
        o.value = __shfl_up((unsigned long long)v.value, d, 64);
        if (l >= d) v = auc_seg_combine(o, v);
    }
    auc_seg ex;
    ex.flag = __shfl_up(v.flag, 1, 64);
    ex.value = __shfl_up((unsigned long long)v.value, 1, 64);
    if (l == 0) ex = auc_seg{0u, 0u};
    __syncthreads();                    // earlier readers of lds are done
    if (l == 63) lds[w] = v;
    __syncthreads();
    auc_seg before{0u, 0u};
    for (int i = 0; i < w; i++) before = auc_seg_combine(before, lds[i]);
    return auc_seg_combine(before, ex);
}

__global__ __launch_bounds__(WG) void auc_terms_kernel(const uint64_t* __restrict__ keys, int64_t n, int nt,
                                                       const ap_tile_rec* __restrict__ recs,
                                                       unsigned long long* __restrict__ two_u) {
    __shared__ uint32_t s_add[WG / 64];
    __shared__ auc_seg s_seg[WG / 64];
    __shared__ uint64_t s_carry;
    __shared__ uint64_t s_sum[WG / 64];
    const int j = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const uint64_t* seg = keys + (size_t)j * n;
    const ap_tile_rec* rj = recs + (size_t)j * nt;
    const int64_t tile0 = (int64_t)b * TILE;

    // positives before the tile
    uint32_t before = 0, tp0;
    for (int i = tid; i < b; i += WG) before += rj[i].pos;
    (void)ap_block_scan_add(before, s_add, &tp0);
    // what the tiles before hold of the group that straddles the tile's start: their tails, backwards up to the tile in
    // which the group began (tile 0's tail always began there: position 0 starts a group)
    if (tid == 0) {
        uint64_t carry = 0;
        if (b > 0 && (seg[tile0] >> 1) == (seg[tile0 - 1] >> 1))
            for (int i = b - 1; i >= 0; i--) {
                carry += ((uint64_t)rj[i].tail_len << 32) | rj[i].tail_pos;
                if (rj[i].tail_began) break;
            }
        s_carry = carry;
    }
    const ap_keys a = ap_load(seg, n, tile0);
    auc_seg v{0u, 0u};
    uint32_t pos = 0;
    {
        uint64_t prev = a.prev;
#pragma unroll
        for (int e = 0; e < IPT; e++) {
            if (a.first + e < n) {
                const uint32_t y = (uint32_t)(a.k[e] & 1u);
                if (a.first + e == 0 || (a.k[e] >> 1) != (prev >> 1)) { v.flag = 1u; v.value = 0u; }
                v.value += AUC_ONE | y;
                pos += y;
            }
            prev = a.k[e];
        }
    }
    uint32_t dummy;
    const uint32_t tp_incl = ap_block_scan_add(pos, s_add, &dummy);   // (its barriers publish s_carry)
    const auc_seg ex = auc_block_exscan_seg(v, s_seg);
    uint64_t tp = (uint64_t)tp0 + tp_incl - pos;
    uint64_t grp = ex.flag ? ex.value : ex.value + s_carry;

    uint64_t acc = 0;
    uint64_t prev = a.prev;
    const uint64_t next_far = a.first + IPT < n ? seg[a.first + IPT] : 0;
#pragma unroll
    for (int e = 0; e < IPT; e++) {
        const int64_t p = a.first + e;
        if (p < n) {
            const uint32_t y = (uint32_t)(a.k[e] & 1u);
            if (p == 0 || (a.k[e] >> 1) != (prev >> 1)) grp = 0;
            grp += AUC_ONE | y;
            tp += y;
            const uint64_t nx = e + 1 < IPT ? a.k[e + 1] : next_far;
            if (p == n - 1 || (nx >> 1) != (a.k[e] >> 1)) {
                const uint64_t gp = grp & 0xffffffffu, len = grp >> 32;   // tp_{g-1} = tp - gp
                acc += (len - gp) * (2 * tp - gp);
            }
        }
        prev = a.k[e];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor((unsigned long long)acc, d, 64);
    if ((tid & 63) == 0) s_sum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        uint64_t t = 0;
        for (int i = 0; i < WG / 64; i++) t += s_sum[i];
        if (t) atomicAdd(two_u + j, (unsigned long long)t);
    }
}

__global__ void auc_finish_kernel(const ap_tile_rec* __restrict__ recs, int nt, int cc, int64_t n,
                                  const int64_t* __restrict__ two_u, double* __restrict__ auc, int64_t* __restrict__ n_pos) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cc) return;
    int64_t P = 0;
    for (int i = 0; i < nt; i++) P += recs[(size_t)j * nt + i].pos;
    const int64_t N = n - P;
    n_pos[j] = P;
    auc[j] = P > 0 && N > 0 ? (double)two_u[j] / (double)(2 * P * N) : __longlong_as_double(0x7ff8000000000000LL);
}

// ---- threshold counts ----------------------------------------------------------------------------------------
constexpr int TC_CLASSES = 1024;    // classes whose three counters a workgroup keeps in LDS (12 KiB)
constexpr int TC_ELEMS = 4096;      // elements per step of a workgroup (whole rows of its classes; at least one)
constexpr int TC_MAX_BLOCKS = 1024; // workgroups per chunk of classes: each one flushes its counters once
constexpr int TC_BATCH = 4;         // elements a thread loads before it counts them (loads in flight)

__global__ __launch_bounds__(WG) void tc_count_kernel(const float* __restrict__ scores, int64_t ld_scores,
                                                      const float* __restrict__ labels, int64_t ld_labels, int64_t n, int c,
                                                      uint32_t thr_key, int rows_per_step,
                                                      unsigned long long* __restrict__ counts, int32_t* __restrict__ flags) {
    __shared__ uint32_t s_cnt[3][TC_CLASSES];
    const int c0 = blockIdx.y * TC_CLASSES;
    const int cn = c - c0 < TC_CLASSES ? c - c0 : TC_CLASSES;
    for (int j = threadIdx.x; j < cn; j += WG) s_cnt[0][j] = s_cnt[1][j] = s_cnt[2][j] = 0u;
    __syncthreads();
    // an element index e of a step is (row e / cn, class e % cn); a thread's next one is WG further on
    const int step_r = WG / cn, step_j = WG % cn;
    int bad = 0;
    for (int64_t row0 = (int64_t)blockIdx.x * rows_per_step; row0 < n; row0 += (int64_t)gridDim.x * rows_per_step) {
        const int64_t left = n - row0;
        const int rows = (int)(left < rows_per_step ? left : rows_per_step);
        int r = (int)threadIdx.x / cn, j = (int)threadIdx.x % cn;
        while (r < rows) {
            int rr[TC_BATCH], jj[TC_BATCH];
            uint32_t sb[TC_BATCH], yb[TC_BATCH];
#pragma unroll
            for (int u = 0; u < TC_BATCH; u++) {
                rr[u] = r;
                jj[u] = j;
                r += step_r;
                j += step_j;
                if (j >= cn) { j -= cn; r++; }
            }
#pragma unroll
            for (int u = 0; u < TC_BATCH; u++)
                if (rr[u] < rows) {
                    const int64_t i = row0 + rr[u];
                    sb[u] = __float_as_uint(scores[i * ld_scores + c0 + jj[u]]);
                    yb[u] = __float_as_uint(labels[i * ld_labels + c0 + jj[u]]);
                }
#pragma unroll
            for (int u = 0; u < TC_BATCH; u++)
                if (rr[u] < rows) {
                    // (on the bit patterns, as ap_pack_kernel: the verdicts do not depend on the kernel's denormal mode)
                    const bool one = yb[u] == 0x3f800000u;
                    if ((sb[u] & 0x7f800000u) == 0x7f800000u) bad |= 1;
                    if (!one && (yb[u] & 0x7fffffffu) != 0u) bad |= 2;
                    const bool hit = ap_desc_key(__uint_as_float(sb[u])) < thr_key;   // score > threshold (descending keys)
                    if (hit | one) atomicAdd(&s_cnt[hit ? (one ? 0 : 1) : 2][jj[u]], 1u);
                }
        }
    }
    if (bad) atomicOr(flags, bad);
    __syncthreads();
    for (int j = threadIdx.x; j < cn; j += WG)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t v = s_cnt[k][j];
            if (v) atomicAdd(counts + (size_t)(c0 + j) * 3 + k, (unsigned long long)v);
        }
}

}  // namespace

extern "C" int at_ranking_metrics_f32(at_ctx* ctx, const float* scores, int64_t ld_scores, const float* labels,
                                      int64_t ld_labels, int64_t n, int c, double* ap, double* map, double* auc,
                                      int64_t* two_u, int64_t* n_pos, double* mauc, int32_t* flags, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ap_plan plan;
    int rc = ap_begin(ctx, "at_ranking_metrics_f32", ld_scores, ld_labels, n, c, stream, &plan);
    if (rc) return rc;
    AT_REQUIRE(scores && labels && auc && two_u && n_pos && mauc && flags, "at_ranking_metrics_f32: null pointer");
    AT_REQUIRE((ap == nullptr) == (map == nullptr), "at_ranking_metrics_f32: ap and map go together");
    AT_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), stream));
    AT_HIP(hipMemsetAsync(two_u, 0, sizeof(int64_t) * (size_t)c, stream));
    for (int c0 = 0; c0 < c; c0 += plan.cc) {
        const int cn = c - c0 < plan.cc ? c - c0 : plan.cc;
        const uint64_t* sorted;
        if ((rc = ap_sorted_chunk(ctx, plan, scores, ld_scores, labels, ld_labels, n, c0, cn, flags, stream, &sorted))) return rc;
        if (ap && (rc = ap_chunk_terms(plan, sorted, n, cn, ap + c0, n_pos + c0, stream))) return rc;
        AT_LAUNCH(auc_terms_kernel, dim3((unsigned)plan.nt, (unsigned)cn), dim3(WG), 0, stream, sorted, n, plan.nt, plan.recs,
                  reinterpret_cast<unsigned long long*>(two_u + c0));
        AT_LAUNCH(auc_finish_kernel, dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, stream, plan.recs, plan.nt, cn, n,
                  two_u + c0, auc + c0, n_pos + c0);
    }
    // both means in one launch, side by side (ap_mean_kernel is one thread walking the classes)
    AT_LAUNCH(ap_mean_kernel, dim3(ap ? 2 : 1), dim3(64), 0, stream, ap_mean_job{auc, n, mauc}, ap_mean_job{ap, -1, map},
              n_pos, c);
    return ap_end(ctx, stream);
}

extern "C" int at_threshold_counts_f32(at_ctx* ctx, const float* scores, int64_t ld_scores, const float* labels,
                                       int64_t ld_labels, int64_t n, int c, float threshold, int64_t* counts,
                                       int32_t* flags, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx != nullptr, "at_threshold_counts_f32: null context");
    AT_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && c >= 1 && c <= 32768, "at_threshold_counts_f32: bad sizes (n = %lld, c = %d)",
               (long long)n, c);
    AT_REQUIRE(ld_scores >= c && ld_labels >= c, "at_threshold_counts_f32: row strides (%lld, %lld) below c = %d",
               (long long)ld_scores, (long long)ld_labels, c);
    AT_REQUIRE(scores && labels && counts && flags, "at_threshold_counts_f32: null pointer");
    AT_REQUIRE(std::isfinite(threshold), "at_threshold_counts_f32: the threshold is not finite");
    AT_HIP(hipSetDevice(ctx->device));
    AT_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), stream));
    AT_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * 3 * (size_t)c, stream));
    // ap_desc_key on the host: the threshold's place among the descending keys (-0.0 is +0.0)
    uint32_t u;
    std::memcpy(&u, &threshold, sizeof u);
    if ((u & 0x7fffffffu) == 0u) u = 0u;
    const uint32_t thr_key = ~(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));
    const int chunks = (c + TC_CLASSES - 1) / TC_CLASSES;
    const int widest = c < TC_CLASSES ? c : TC_CLASSES;
    const int rows_per_step = widest >= TC_ELEMS ? 1 : TC_ELEMS / widest;
    const int64_t steps = (n + rows_per_step - 1) / rows_per_step;
    const unsigned blocks = (unsigned)(steps < TC_MAX_BLOCKS ? steps : TC_MAX_BLOCKS);
    AT_LAUNCH(tc_count_kernel, dim3(blocks, (unsigned)chunks), dim3(WG), 0, stream, scores, ld_scores, labels, ld_labels, n, c,
              thr_key, rows_per_step, reinterpret_cast<unsigned long long*>(counts), flags);
    return AT_OK;
}
