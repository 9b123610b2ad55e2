// ap_stages.h -- the stages that at_average_precision_f32 (average_precision.hip) and at_ranking_metrics_f32
// (ranking_metrics.hip) share: one key per (sample, class), one keys-only sort per chunk of classes, and the tile records
// behind it.  Both metrics are sums over the groups of equal scores of a class in descending score order, so both walk
// the same sorted keys with the same group boundaries.
//
// Layout.  The classes are processed in chunks of cc so that the two key buffers of a chunk stay within the workspace
// budget (switch ap_ws_mb).  Per chunk:
//   1. ap_pack_kernel reads the [n][cc] block of scores and labels as it lies (rows of cc consecutive floats) and writes
//      one 64-bit key per element: class_in_chunk << 33 | desc_key(score) << 1 | label.  desc_key is the order-preserving
//      flip of the float's bits, inverted (higher scores first), of the score with -0.0 made +0.0.  It raises the flags.
//      (No transpose: a keys-only sort does not care where a key starts out.)
//   2. a keys-only onesweep radix sort over bits [1, 33 + ceil(log2 cc)).  Every class has n keys, so class j's sorted
//      segment is [j n, (j + 1) n) -- no offsets.  The label bit is not sorted on: within a group the order is irrelevant.
//   3. ap_tile_kernel: per (class, tile of 2048 positions), the positives of the tile, and the positives and the length
//      of the tile's last group (the run of equal scores that reaches the tile's end; it may have begun many tiles before).
// (ap_sorted_chunk does the three.)  Behind them:
//   4. ap_terms_kernel: per (class, tile), tp before the tile and P from the tile counts (integers: any order is exact), a
//      block scan for tp at every position, a segmented block scan for the positives of the group so far (seeded, for the
//      group that straddles the tile's start, by walking the earlier tiles' tail records backwards), and the terms of
//      the groups that END in the tile, added per thread in position order and then by a fixed tree -> partial[class][tile].
//   5. ap_finish_kernel: one thread per class adds the partials in ascending tile order.
// (ap_chunk_terms does the two; ranking_metrics.hip has their counterparts for the ROC AUC.)  At the end ap_mean_kernel
// adds the per-class values over the classes where they are defined in ascending class order (compensated, so that the
// sum is the rounded exact sum).  The tiles are relative to the class's segment, so the order of every fp64 addition
// depends on n and the data alone: the bits do not depend on the chunking, and no float atomic is used anywhere.
#pragma once
#include <cmath>
#include <cstring>

#include "at_internal.h"
#include "at_sort.h"

namespace {

constexpr int WG = 256;
constexpr int IPT = 8;             // positions per thread of the tile kernels
constexpr int TILE = WG * IPT;     // positions per tile
constexpr int PACK_ELEMS = 4096;   // elements per workgroup of the pack kernel (whole rows; at least one)

__device__ __forceinline__ uint32_t ap_desc_key(float s) {
    uint32_t u = __float_as_uint(s);
    if ((u & 0x7fffffffu) == 0u) u = 0u;                         // -0.0 and +0.0 are one group (denormals are not zero)
    const uint32_t asc = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
    return ~asc;
}

__global__ __launch_bounds__(WG) void ap_pack_kernel(const float* __restrict__ scores, int64_t ld_scores,
                                                     const float* __restrict__ labels, int64_t ld_labels, int64_t n, int c0,
                                                     int cc, int rows_per_block, uint64_t* __restrict__ keys,
                                                     int32_t* __restrict__ flags) {
    const int64_t row0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t left = n - row0;
    const int rows = (int)(left < rows_per_block ? left : rows_per_block);
    const int64_t count = (int64_t)rows * cc;                    // (cc above PACK_ELEMS: one row of any length)
    int bad = 0;
    for (unsigned e = threadIdx.x; e < (unsigned)count; e += WG) {   // (count <= max(PACK_ELEMS, cc): 32-bit division)
        const int r = (int)(e / (unsigned)cc);
        const int j = (int)(e - (unsigned)r * (unsigned)cc);
        const int64_t i = row0 + r;
        const float s = scores[i * ld_scores + c0 + j];
        const float y = labels[i * ld_labels + c0 + j];
        // (on the bit patterns: the verdicts do not depend on the kernel's denormal mode)
        const uint32_t sb = __float_as_uint(s), yb = __float_as_uint(y);
        const uint32_t one = yb == 0x3f800000u ? 1u : 0u;
        if ((sb & 0x7f800000u) == 0x7f800000u) bad |= 1;          // NaN or infinity
        if (!one && (yb & 0x7fffffffu) != 0u) bad |= 2;           // neither 1.0 nor a zero
        keys[(size_t)i * cc + j] = ((uint64_t)j << 33) | ((uint64_t)ap_desc_key(s) << 1) | one;
    }
    if (bad) atomicOr(flags, bad);
}

// inclusive scans over the workgroup, thread order (wave shuffles, then the four wave totals through LDS)
__device__ __forceinline__ uint32_t ap_block_scan_add(uint32_t v, uint32_t* lds /*[WG / 64]*/, uint32_t* total) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (l >= d) v += o;
    }
    __syncthreads();                    // earlier readers of lds are done
    if (l == 63) lds[w] = v;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < WG / 64; i++) {
        const uint32_t t = lds[i];
        if (i < w) before += t;
        all += t;
    }
    *total = all;
    return v + before;
}

// Segmented sum: an element is (flag, value); flag = a group starts inside the element's span, value = positives since
// the last start (or since the span's beginning).  combine(a, b) = b.flag ? b : (a.flag, a.value + b.value).
struct ap_seg { uint32_t flag, value; };
__device__ __forceinline__ ap_seg ap_seg_combine(ap_seg a, ap_seg b) {
    ap_seg r;
    r.flag = a.flag | b.flag;
    r.value = b.flag ? b.value : a.value + b.value;
    return r;
}
__device__ __forceinline__ ap_seg ap_block_scan_seg(ap_seg v, ap_seg* lds /*[WG / 64]*/) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        ap_seg o;
        o.flag = __shfl_up(v.flag, d, 64);
        o.value = __shfl_up(v.value, d, 64);
        if (l >= d) v = ap_seg_combine(o, v);
    }
    __syncthreads();
    if (l == 63) lds[w] = v;
    __syncthreads();
    ap_seg before{0u, 0u};
    for (int i = 0; i < w; i++) before = ap_seg_combine(before, lds[i]);
    return ap_seg_combine(before, v);
}

// what a tile leaves for the others: its positives, the positives of the group that reaches its end, whether that
// group began inside it, and how many of the tile's positions it takes
struct ap_tile_rec { uint32_t pos, tail_pos, tail_began, tail_len; };

// loads a thread's IPT keys of (segment, tile) and the key in front of the first one
struct ap_keys {
    uint64_t k[IPT];
    uint64_t prev;       // key at position first - 1 (undefined when first == 0)
    int64_t first;       // position of k[0] in the segment
};
__device__ __forceinline__ ap_keys ap_load(const uint64_t* __restrict__ seg, int64_t n, int64_t tile0) {
    ap_keys r;
    r.first = tile0 + (int64_t)threadIdx.x * IPT;
#pragma unroll
    for (int e = 0; e < IPT; e++) r.k[e] = r.first + e < n ? seg[r.first + e] : 0;
    r.prev = (r.first > 0 && r.first - 1 < n) ? seg[r.first - 1] : 0;
    return r;
}

// a thread's span as a segmented-scan element; *pos: its positives; *since: its positions from the last start on (all of
// them when no group starts inside the span)
__device__ __forceinline__ ap_seg ap_span(const ap_keys& a, int64_t n, uint32_t* pos, uint32_t* since) {
    ap_seg v{0u, 0u};
    uint32_t p = 0, len = 0;
    uint64_t prev = a.prev;
#pragma unroll
    for (int e = 0; e < IPT; e++) {
        if (a.first + e < n) {
            const uint32_t y = (uint32_t)(a.k[e] & 1u);
            if (a.first + e == 0 || (a.k[e] >> 1) != (prev >> 1)) { v.flag = 1u; v.value = 0u; len = 0; }
            v.value += y;
            p += y;
            len++;
        }
        prev = a.k[e];
    }
    *pos = p;
    *since = len;
    return v;
}

__global__ __launch_bounds__(WG) void ap_tile_kernel(const uint64_t* __restrict__ keys, int64_t n, int nt,
                                                     ap_tile_rec* __restrict__ recs) {
    __shared__ uint32_t s_add[WG / 64];
    __shared__ ap_seg s_seg[WG / 64];
    const int j = blockIdx.y, b = blockIdx.x;
    const ap_keys a = ap_load(keys + (size_t)j * n, n, (int64_t)b * TILE);
    uint32_t pos, since;
    const ap_seg v = ap_span(a, n, &pos, &since);
    uint32_t total;
    (void)ap_block_scan_add(pos, s_add, &total);
    const ap_seg s = ap_block_scan_seg(v, s_seg);
    // the tail group's length: the same segmented sum over the positions instead of the positives
    const ap_seg t = ap_block_scan_seg(ap_seg{v.flag, since}, s_seg);
    if (threadIdx.x == WG - 1) recs[(size_t)j * nt + b] = ap_tile_rec{total, s.value, s.flag, t.value};
}

__global__ __launch_bounds__(WG) void ap_terms_kernel(const uint64_t* __restrict__ keys, int64_t n, int nt,
                                                      const ap_tile_rec* __restrict__ recs, double* __restrict__ partial) {
    __shared__ uint32_t s_add[WG / 64];
    __shared__ ap_seg s_seg[WG / 64];
    __shared__ uint32_t s_carry;
    __shared__ double s_sum[WG];
    const int j = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const uint64_t* seg = keys + (size_t)j * n;
    const ap_tile_rec* rj = recs + (size_t)j * nt;
    const int64_t tile0 = (int64_t)b * TILE;

    // positives before the tile, and in the class (integers: exact in any order)
    uint32_t before = 0, all = 0;
    for (int i = tid; i < nt; i += WG) {
        const uint32_t p = rj[i].pos;
        all += p;
        if (i < b) before += p;
    }
    uint32_t P, tp0, dummy;
    {
        const uint32_t incl = ap_block_scan_add(all, s_add, &P);
        (void)incl;
        (void)ap_block_scan_add(before, s_add, &tp0);
    }
    // positives of the group that straddles the tile's start, in the tiles before: the tails of the earlier tiles,
    // backwards up to the tile in which the group began
    if (tid == 0) {
        uint32_t carry = 0;
        if (b > 0 && (seg[tile0] >> 1) == (seg[tile0 - 1] >> 1))
            for (int i = b - 1; i >= 0; i--) {
                carry += rj[i].tail_pos;
                if (rj[i].tail_began) break;
            }
        s_carry = carry;
    }
    const ap_keys a = ap_load(seg, n, tile0);
    uint32_t pos, since;
    const ap_seg v = ap_span(a, n, &pos, &since);
    (void)since;
    const uint32_t tp_incl = ap_block_scan_add(pos, s_add, &dummy);   // (its barriers publish s_carry)
    const ap_seg s_incl = ap_block_scan_seg(v, s_seg);
    // exclusive values: the state in front of this thread's first position
    uint32_t tp = tp0 + tp_incl - pos;
    ap_seg ex;
    ex.flag = __shfl_up(s_incl.flag, 1, 64);
    ex.value = __shfl_up(s_incl.value, 1, 64);
    __syncthreads();
    if ((tid & 63) == 63) s_seg[tid >> 6] = s_incl;
    __syncthreads();
    if ((tid & 63) == 0) ex = tid == 0 ? ap_seg{0u, 0u} : s_seg[(tid >> 6) - 1];
    // positives of the current group so far: since its start inside the tile, else with what the earlier tiles hold
    uint32_t grp = ex.flag ? ex.value : ex.value + s_carry;

    const double Pd = (double)P;
    double acc = 0.0;
    uint64_t prev = a.prev;
    const uint64_t next_far = a.first + IPT < n ? seg[a.first + IPT] : 0;
#pragma unroll
    for (int e = 0; e < IPT; e++) {
        const int64_t p = a.first + e;
        if (p < n) {
            const uint32_t y = (uint32_t)(a.k[e] & 1u);
            if (p == 0 || (a.k[e] >> 1) != (prev >> 1)) grp = 0;
            grp += y;
            tp += y;
            const uint64_t nx = e + 1 < IPT ? a.k[e + 1] : next_far;
            const bool end = p == n - 1 || (nx >> 1) != (a.k[e] >> 1);
            if (end && grp != 0)
                acc += ((double)grp / Pd) * ((double)tp / (double)(p + 1));
        }
        prev = a.k[e];
    }
    // fixed tree over the threads
    s_sum[tid] = acc;
    __syncthreads();
    for (int h = WG / 2; h >= 1; h >>= 1) {
        if (tid < h) s_sum[tid] = s_sum[tid] + s_sum[tid + h];
        __syncthreads();
    }
    if (tid == 0) partial[(size_t)j * nt + b] = s_sum[0];
}

__global__ void ap_finish_kernel(const ap_tile_rec* __restrict__ recs, const double* __restrict__ partial, int nt, int cc,
                                 double* __restrict__ ap, int64_t* __restrict__ n_pos) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cc) return;
    int64_t P = 0;
    double s = 0.0;
    for (int i = 0; i < nt; i++) {
        P += recs[(size_t)j * nt + i].pos;
        s += partial[(size_t)j * nt + i];
    }
    n_pos[j] = P;
    ap[j] = P > 0 ? s : __longlong_as_double(0x7ff8000000000000LL);
}

// map[0] = the fp64 sum of ap over the classes with positives, ascending, with the rounding errors of the additions
// carried along (Neumaier) and added at the end: the rounded exact sum; map[1] = their number.  (all_pos: a class with
// that many positives is left out as well -- the ROC AUC passes n, the average precision -1.  Workgroup 0 does `first`,
// workgroup 1, where launched, `second`.)
struct ap_mean_job {
    const double* ap;
    int64_t all_pos;
    double* map;
};
__global__ void ap_mean_kernel(ap_mean_job first, ap_mean_job second, const int64_t* __restrict__ n_pos, int c) {
    if (blockIdx.x > 1 || threadIdx.x != 0) return;
    const double* __restrict__ ap = blockIdx.x ? second.ap : first.ap;
    const int64_t all_pos = blockIdx.x ? second.all_pos : first.all_pos;
    double* __restrict__ map = blockIdx.x ? second.map : first.map;
    double s = 0.0, comp = 0.0;
    int64_t m = 0;
    for (int j = 0; j < c; j++)
        if (n_pos[j] > 0 && n_pos[j] != all_pos) {
            const double x = ap[j];
            const double t = s + x;
            comp += fabs(s) >= fabs(x) ? (s - t) + x : (x - t) + s;
            s = t;
            m++;
        }
    map[0] = s + comp;
    map[1] = (double)m;
}

size_t ap_align(size_t b) { return (b + 255) & ~size_t(255); }

int ap_ceil_log2(int v) {
    int b = 0;
    while (((int64_t)1 << b) < v) b++;
    return b;
}

// ---- host side ------------------------------------------------------------------------------------------------
// The chunking of a call and its workspace (WS_AVG_PRECISION: the two key buffers of a chunk, tile records, tile partials).
struct ap_plan {
    int cc, nt;               // classes per chunk, tiles per class
    uint64_t *keys_a, *keys_b;
    ap_tile_rec* recs;        // [cc][nt]
    double* partial;          // [cc][nt]
};

// Checks the sizes (who: the entry's name, for the messages), chooses the chunk, makes the stream wait for the context's
// previous call where that ran on another stream, and sizes the workspace.
int ap_begin(at_ctx* ctx, const char* who, int64_t ld_scores, int64_t ld_labels, int64_t n, int c, hipStream_t stream,
             ap_plan* plan) {
    AT_REQUIRE(ctx != nullptr, "%s: null context", who);
    AT_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && c >= 1, "%s: bad sizes (n = %lld, c = %d)", who, (long long)n, c);
    AT_REQUIRE(ld_scores >= c && ld_labels >= c, "%s: row strides (%lld, %lld) below c = %d", who, (long long)ld_scores,
               (long long)ld_labels, c);
    AT_HIP(hipSetDevice(ctx->device));
    // classes per chunk: two key buffers of n * cc keys within the budget, at least one class
    // (switch ap_ws_mb: MiB; a negative value is a test hook and gives that many classes per chunk)
    const int ws_mb = ctx->dbg.ap_ws_mb;
    int64_t cc64 = ws_mb < 0 ? -(int64_t)ws_mb : ((int64_t)(ws_mb > 0 ? ws_mb : 1024) << 20) / (16 * n);
    if (cc64 < 1) cc64 = 1;
    if (cc64 > c) cc64 = c;
    if (cc64 > 32768) cc64 = 32768;   // (the class is the launch grid's y index)
    const int cc = (int)cc64;
    AT_REQUIRE((int64_t)cc * n < ((int64_t)1 << 32), "%s: n = %lld is too large for one sort", who, (long long)n);
    const int nt = (int)((n + TILE - 1) / TILE);
    const size_t nkeys = (size_t)n * cc;
    const size_t b_keys = ap_align(8 * nkeys), b_recs = ap_align(sizeof(ap_tile_rec) * (size_t)cc * nt),
                 b_part = ap_align(8 * (size_t)cc * nt);
    // The slots are the context's: a call on another stream than the previous one waits for it (at_sum_f32's rule).
    { const int rc = at_guard_enter(&ctx->guard[AT_GUARD_AP], stream); if (rc) return rc; }
    unsigned char* w = static_cast<unsigned char*>(at_ws(ctx, WS_AVG_PRECISION, 2 * b_keys + b_recs + b_part, stream));
    if (!w) return AT_E_NOMEM;
    plan->cc = cc;
    plan->nt = nt;
    plan->keys_a = reinterpret_cast<uint64_t*>(w);
    plan->keys_b = reinterpret_cast<uint64_t*>(w + b_keys);
    plan->recs = reinterpret_cast<ap_tile_rec*>(w + 2 * b_keys);
    plan->partial = reinterpret_cast<double*>(w + 2 * b_keys + b_recs);
    return AT_OK;
}

// Stages 1-3 for the cn classes from c0 on: *sorted = their sorted keys, plan.recs = their tile records.
int ap_sorted_chunk(at_ctx* ctx, const ap_plan& plan, const float* scores, int64_t ld_scores, const float* labels,
                    int64_t ld_labels, int64_t n, int c0, int cn, int32_t* flags, hipStream_t stream,
                    const uint64_t** sorted) {
    const int rows_per_block = cn >= PACK_ELEMS ? 1 : PACK_ELEMS / cn;
    const unsigned pack_blocks = (unsigned)((n + rows_per_block - 1) / rows_per_block);
    AT_LAUNCH(ap_pack_kernel, dim3(pack_blocks), dim3(WG), 0, stream, scores, ld_scores, labels, ld_labels, n, c0, cn,
              rows_per_block, plan.keys_a, flags);
    rocprim::double_buffer<uint64_t> kb(plan.keys_a, plan.keys_b);
    const int rc = at_sort_keys(ctx, WS_AVG_PRECISION_TMP, kb, (size_t)n * cn, 1u, 33u + (unsigned)ap_ceil_log2(cn), stream);
    if (rc) return rc;
    *sorted = kb.current();
    AT_LAUNCH(ap_tile_kernel, dim3((unsigned)plan.nt, (unsigned)cn), dim3(WG), 0, stream, *sorted, n, plan.nt, plan.recs);
    return AT_OK;
}

// Stages 4-5 for a chunk: ap, n_pos point at the chunk's first class.
int ap_chunk_terms(const ap_plan& plan, const uint64_t* sorted, int64_t n, int cn, double* ap, int64_t* n_pos,
                   hipStream_t stream) {
    AT_LAUNCH(ap_terms_kernel, dim3((unsigned)plan.nt, (unsigned)cn), dim3(WG), 0, stream, sorted, n, plan.nt, plan.recs,
              plan.partial);
    AT_LAUNCH(ap_finish_kernel, dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, stream, plan.recs, plan.partial, plan.nt, cn,
              ap, n_pos);
    return AT_OK;
}

// behind the call's last launch
int ap_end(at_ctx* ctx, hipStream_t stream) { return at_guard_leave(&ctx->guard[AT_GUARD_AP], stream); }

}  // namespace
