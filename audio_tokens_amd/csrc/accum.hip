// accum.hip -- compute_centroids (accumulate) of one Lloyd iteration on gfx950: at_centroid_accum_f32.
//
// compute_centroids must reproduce what FAISS's owning thread produces: the members of a cluster
// are added in ASCENDING point index with fp32 adds.  That order is made explicit here: a stable
// radix sort of (assignment, point index) pairs (rocPRIM) yields every cluster's member list in
// ascending index; one wavefront then walks one list, lanes across the feature axis, so each
// row is one coalesced 4d-byte read and the adds are sequential per (cluster, feature) exactly as
// on the CPU.  No float atomics anywhere: results are bitwise reproducible.
//
// The kernels that sum (and the sort keys and segment starts) are in accum_kernels.h, shared with the
// weighted sums of waccum.hip; this file instantiates their WEIGHTED = false forms.  Here: the kernels
// that build member lists ahead of or without the sort, then the host driver that queues everything
// (one plan, two ways to build the member lists, one exit); DESIGN.md, "Host driver of the centroid
// sums", maps its stages to streams.
#include <cstdlib>
#include <cstring>

#include "accum_kernels.h"
#include "at_internal.h"
#include "at_sort.h"

namespace {

constexpr int EARLY_ROWS = 4096;    // rows per workgroup of the ordered compaction

// The three carved-up workspaces.  Each view is filled by its fetch(): the slot from at_ws, zeroed on `clear_on` when
// it is new (at_ws puts long_pred_k / buckets_k back to 0 when it allocates) or was last laid out for another k.
// WS_LONG_PRED, in ints: [0] number of long clusters the last call saw (the next call's early set, capped at
// EARLY_MAX), [1 .. EARLY_MAX] their ids, then k generation marks ("summed early in call `gen`").  One definition for
// all users: round 2 raised EARLY_MAX from 8 to 16 and left the marks at offset 16, on top of the last id.
struct LongPred {
    int *pred_n, *pred;
    unsigned* done;
    static constexpr size_t MARKS_AT = 1 + EARLY_MAX;
    static size_t bytes(int k) { return (MARKS_AT + (size_t)k) * sizeof(int); }
    int fetch(at_ctx* ctx, int k, hipStream_t clear_on) {
        int* pw = static_cast<int*>(at_ws(ctx, WS_LONG_PRED, bytes(k), clear_on));
        if (!pw) return AT_E_NOMEM;
        if (ctx->long_pred_k != k) {   // no predictions, no marks
            AT_HIP(hipMemsetAsync(pw, 0, bytes(k), clear_on));
            ctx->long_pred_k = k;
            ctx->long_gen = 0;
        }
        pred_n = pw, pred = pw + 1, done = reinterpret_cast<unsigned*>(pw + MARKS_AT);
        return AT_OK;
    }
};
static_assert(LongPred::MARKS_AT >= 1 + EARLY_MAX, "the generation marks must start behind the last predicted cluster id");

// WS_BUCKETS, in words: counts[k+1] (zero between calls: the scan clears what it has read) | cursor[k+1] | longs[k+2]
struct BucketTable {
    unsigned *counts, *cursor;
    int* longs;
    static size_t bytes(int k) { return ((size_t)3 * k + 8) * 4; }
    int fetch(at_ctx* ctx, int k, hipStream_t clear_on) {
        unsigned* bw = static_cast<unsigned*>(at_ws(ctx, WS_BUCKETS, bytes(k), clear_on));
        if (!bw) return AT_E_NOMEM;
        if (ctx->buckets_k != k) {
            AT_HIP(hipMemsetAsync(bw, 0, bytes(k), clear_on));
            ctx->buckets_k = k;
        }
        counts = bw, cursor = bw + (k + 1), longs = reinterpret_cast<int*>(bw + 2 * (k + 1));
        return AT_OK;
    }
};

// WS_LONG_EARLY, in words: blockcnt[EARLY_MAX][nblk] | blockbase[EARLY_MAX][nblk] | eoff[EARLY_MAX + 1] | lists[n]
// (the bucket strategy writes its lists straight into the clusters' segments: the last part is its rank sort's scratch)
struct EarlyLists {
    uint32_t *blockcnt, *blockbase, *eoff, *lists;
    static size_t bytes(int nblk, size_t n) { return ((size_t)2 * EARLY_MAX * nblk + EARLY_MAX + 1 + n) * 4; }
    int fetch(at_ctx* ctx, int nblk, size_t n, hipStream_t stream) {
        blockcnt = static_cast<uint32_t*>(at_ws(ctx, WS_LONG_EARLY, bytes(nblk, n), stream));
        if (!blockcnt) return AT_E_NOMEM;
        blockbase = blockcnt + (size_t)EARLY_MAX * nblk, eoff = blockbase + (size_t)EARLY_MAX * nblk, lists = eoff + EARLY_MAX + 1;
        return AT_OK;
    }
};

// ---- member lists of the (predicted) long clusters, ahead of the sort -----------------------------------------
// A list of tens of thousands of members is one dependent chain of adds, 300 us at 2 M rows: as long as everything
// else of the accumulation together, and it used to start only after the sort.  The clusters that were long in
// the previous call (a Lloyd iteration changes 2 % of the assignments) get their lists from an ordered compaction
// of ids instead -- count per 4096-row block, scan, ordered write: three small launches -- so their chains run
// beside the sort.  Whatever the prediction, a list built here is exactly the cluster's members in ascending row
// order; a cluster that is not long after all is left to the short-list kernel.
__global__ void __launch_bounds__(WG) early_count_kernel(const long* __restrict__ ids, long n, const int* __restrict__ pred,
                                                         const int* __restrict__ pred_n, int nblk,
                                                         uint32_t* __restrict__ blockcnt) {
    __shared__ uint32_t cnt[EARLY_MAX];
    const int np = min(*pred_n, EARLY_MAX);
    if (threadIdx.x < EARLY_MAX) cnt[threadIdx.x] = 0;
    __syncthreads();
    if (np > 0) {
        long want[EARLY_MAX];
#pragma unroll
        for (int m = 0; m < EARLY_MAX; m++) want[m] = m < np ? (long)pred[m] : -2L;
        const long r0 = (long)blockIdx.x * EARLY_ROWS;
        uint32_t mine[EARLY_MAX];
#pragma unroll
        for (int m = 0; m < EARLY_MAX; m++) mine[m] = 0;
        for (int i = threadIdx.x; i < EARLY_ROWS; i += WG) {
            const long r = r0 + i;
            if (r < n) {
                const long id = ids[r];
#pragma unroll
                for (int m = 0; m < EARLY_MAX; m++) mine[m] += id == want[m];
            }
        }
#pragma unroll
        for (int m = 0; m < EARLY_MAX; m++) {
            uint32_t v = mine[m];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(&cnt[m], v);
        }
    }
    __syncthreads();
    if (threadIdx.x < EARLY_MAX) blockcnt[(size_t)threadIdx.x * nblk + blockIdx.x] = cnt[threadIdx.x];
}

// one workgroup: blockbase[m][b] = members of pred[m] in blocks before b; eoff[m] = start of list m (lists back to back)
__global__ void __launch_bounds__(1024) early_scan_kernel(const uint32_t* __restrict__ blockcnt, int nblk,
                                                          uint32_t* __restrict__ blockbase, uint32_t* __restrict__ eoff) {
    __shared__ uint32_t part[EARLY_MAX][1024];
    __shared__ uint32_t total[EARLY_MAX];
    const int t = threadIdx.x;
    const int per = (nblk + 1023) / 1024;
    const int lo = min(nblk, t * per), hi = min(nblk, lo + per);
#pragma unroll
    for (int m = 0; m < EARLY_MAX; m++) {
        uint32_t s = 0;
        for (int b = lo; b < hi; b++) s += blockcnt[(size_t)m * nblk + b];
        part[m][t] = s;
    }
    __syncthreads();
    if (t < EARLY_MAX) {   // (serial scans side by side, over the threads that hold blocks: 64 of them at 262 144 rows)
        const int used = min(1024, (nblk + per - 1) / per);
        uint32_t run = 0;
        for (int i = 0; i < used; i++) { const uint32_t v = part[t][i]; part[t][i] = run; run += v; }
        total[t] = run;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < EARLY_MAX; m++) {
        uint32_t run = part[m][t];
        for (int b = lo; b < hi; b++) {
            blockbase[(size_t)m * nblk + b] = run;
            run += blockcnt[(size_t)m * nblk + b];
        }
    }
    if (t == 0) {
        uint32_t run = 0;
        for (int m = 0; m < EARLY_MAX; m++) { eoff[m] = run; run += total[m]; }
        eoff[EARLY_MAX] = run;
    }
}

// After the sort: every long cluster goes into the next call's early set (pred), those the early pass has not summed
// into late[] (late[0] = how many) -- so that the regular long pass is a handful of workgroups, not k x d/4 of which
// all but a few leave at once (65-95 us of dispatch at k = 8192).
__global__ void __launch_bounds__(WG) long_detect_kernel(const uint32_t* __restrict__ offsets, int k, uint32_t long_list,
                                                         const unsigned* __restrict__ done, unsigned gen,
                                                         int* __restrict__ pred, int* __restrict__ pred_n,
                                                         int* __restrict__ late) {
    const int c = blockIdx.x * WG + threadIdx.x;
    if (c >= k) return;
    if (offsets[c + 1] - offsets[c] <= long_list) return;
    const int slot = atomicAdd(pred_n, 1);
    if (slot < EARLY_MAX) pred[slot] = c;
    if (done[c] != gen) late[1 + atomicAdd(&late[0], 1)] = c;
}

__global__ void __launch_bounds__(WG) early_write_kernel(const long* __restrict__ ids, long n, const int* __restrict__ pred,
                                                         const int* __restrict__ pred_n, int nblk,
                                                         const uint32_t* __restrict__ blockbase,
                                                         const uint32_t* __restrict__ eoff, uint32_t* __restrict__ lists,
                                                         const uint32_t* __restrict__ seg_offsets) {
    // list m starts at eoff[m] (lists back to back), or -- seg_offsets given -- at the cluster's own segment of the
    // member-list array (the bucket path: `lists` is that array)
    __shared__ uint32_t wave_cnt[WG / 64];
    __shared__ uint32_t run[EARLY_MAX];
    const int np = min(*pred_n, EARLY_MAX);
    if (np <= 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < np)
        run[threadIdx.x] = (seg_offsets ? seg_offsets[pred[threadIdx.x]] : eoff[threadIdx.x]) +
                           blockbase[(size_t)threadIdx.x * nblk + blockIdx.x];
    __syncthreads();
    const long r0 = (long)blockIdx.x * EARLY_ROWS;
    for (int i0 = 0; i0 < EARLY_ROWS; i0 += WG) {        // 256 consecutive rows per round, in row order
        const long r = r0 + i0 + threadIdx.x;
        const long id = r < n ? ids[r] : -1L;
        for (int m = 0; m < np; m++) {
            const bool hit = id == (long)pred[m];
            const unsigned long long b = __ballot(hit);
            if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(b);
            __syncthreads();
            uint32_t before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < WG / 64; w++) {
                before += w < wave ? wave_cnt[w] : 0u;
                all += wave_cnt[w];
            }
            if (hit) lists[run[m] + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)r;
            __syncthreads();
            if (threadIdx.x == 0) run[m] += all;
            __syncthreads();
        }
    }
}

// ---- member lists without a radix sort (the bucket path) ------------------------------------------------------
// rocPRIM's onesweep needs eight launches (histogram, two passes, their fills) whatever n is: 107 us of a 0.5 ms
// iteration at the 262 144 rows a rank holds in an 8-GPU run, 130 us at 2 M.  With k <= 16 384 clusters a row's bucket
// is known from its id alone: count per cluster (LDS histogram per 4096-row block), scan, scatter to the cluster's
// segment (slots handed out by LDS atomics: any order), then one wave per cluster restores ascending row order with
// a bitonic sort in LDS -- lists hold 30-250 rows.  Lists longer than 2048 rows never enter the scatter: their
// members come, in order, from the ordered compaction above (now driven by the exact counts of the scan instead
// of a prediction), on the side stream, so their add chains start after two small kernels.
constexpr uint32_t BK_SKIP = 0xffffffffu;

__global__ void __launch_bounds__(WG) bucket_count_kernel(const long* __restrict__ ids, long n, int k, int rows_per_block,
                                                          unsigned* __restrict__ counts) {
    extern __shared__ unsigned bk_h[];   // k + 1 bins (the last one: ids outside [0, k))
    for (int b = threadIdx.x; b <= k; b += WG) bk_h[b] = 0;
    __syncthreads();
    const long r0 = (long)blockIdx.x * rows_per_block;
    for (int i = threadIdx.x; i < rows_per_block; i += WG) {
        const long r = r0 + i;
        if (r < n) {
            const long id = ids[r];
            atomicAdd(&bk_h[(id >= 0 && id < k) ? (int)id : k], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b <= k; b += WG)
        if (bk_h[b]) atomicAdd(&counts[b], bk_h[b]);
}

// one workgroup: offsets (exclusive scan of the k+1 counts, offsets[k+1] = n), cursor = offsets (BK_SKIP for the
// clusters the compaction serves), longs[0] = number of long clusters, longs[1..] = their ids in ascending order
// (the first EARLY_MAX are the compaction's); counts are zeroed for the next call.
__global__ void __launch_bounds__(1024) bucket_scan_kernel(unsigned* __restrict__ counts, int k, uint32_t long_list,
                                                           uint32_t* __restrict__ offsets, unsigned* __restrict__ cursor,
                                                           int* __restrict__ longs) {
    __shared__ uint32_t part[1024], lpart[1024];
    const int t = threadIdx.x;
    const int per = (k + 1 + 1023) / 1024;
    const int lo = min(k + 1, t * per), hi = min(k + 1, lo + per);
    uint32_t s = 0, nl = 0;
    for (int b = lo; b < hi; b++) {
        const uint32_t c = counts[b];
        s += c;
        nl += (b < k && c > long_list) ? 1u : 0u;
    }
    part[t] = s;
    lpart[t] = nl;
    __syncthreads();
    if (t < 64) {   // exclusive scans of the 1024 partial sums: 16 per lane, then across the wave
        uint32_t a[16], la[16], sa = 0, sl = 0;
#pragma unroll
        for (int u = 0; u < 16; u++) { a[u] = part[16 * t + u]; la[u] = lpart[16 * t + u]; sa += a[u]; sl += la[u]; }
        uint32_t xa = sa, xl = sl;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t ya = __shfl_up(xa, off), yl = __shfl_up(xl, off);
            if (t >= off) { xa += ya; xl += yl; }
        }
        uint32_t ra = xa - sa, rl = xl - sl;
#pragma unroll
        for (int u = 0; u < 16; u++) { part[16 * t + u] = ra; lpart[16 * t + u] = rl; ra += a[u]; rl += la[u]; }
        if (t == 63) { offsets[k + 1] = xa; longs[0] = (int)xl; }
    }
    __syncthreads();
    uint32_t run = part[t], lrun = lpart[t];
    for (int b = lo; b < hi; b++) {
        const uint32_t c = counts[b];
        offsets[b] = run;
        const bool is_long = b < k && c > long_list;
        cursor[b] = (is_long && lrun < (uint32_t)EARLY_MAX) ? BK_SKIP : run;
        if (is_long) longs[1 + lrun++] = b;
        run += c;
        counts[b] = 0;
    }
}

__global__ void __launch_bounds__(WG) bucket_scatter_kernel(const long* __restrict__ ids, long n, int k, int rows_per_block,
                                                            unsigned* __restrict__ cursor, uint32_t* __restrict__ order) {
    extern __shared__ unsigned bk_s[];   // cnt[k+1] | base[k+1]
    unsigned* cnt = bk_s;
    unsigned* base = bk_s + (k + 1);
    for (int b = threadIdx.x; b <= k; b += WG) cnt[b] = 0;
    __syncthreads();
    const long r0 = (long)blockIdx.x * rows_per_block;
    for (int i = threadIdx.x; i < rows_per_block; i += WG) {
        const long r = r0 + i;
        if (r < n) {
            const long id = ids[r];
            atomicAdd(&cnt[(id >= 0 && id < k) ? (int)id : k], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b <= k; b += WG) {
        const unsigned c = cnt[b];
        if (c) base[b] = cursor[b] == BK_SKIP ? BK_SKIP : atomicAdd(&cursor[b], c);
        cnt[b] = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows_per_block; i += WG) {
        const long r = r0 + i;
        if (r < n) {
            const long id = ids[r];
            const int b = (id >= 0 && id < k) ? (int)id : k;
            const unsigned bs = base[b];
            if (bs != BK_SKIP) order[bs + atomicAdd(&cnt[b], 1u)] = (uint32_t)r;
        }
    }
}

// one wave per cluster: its 2 .. 2048 members into ascending row order (bitonic sort in LDS, padded with ~0)
__global__ void __launch_bounds__(WG) member_sort_kernel(uint32_t* __restrict__ order, const uint32_t* __restrict__ offsets,
                                                         int k, uint32_t long_list) {
    __shared__ uint32_t ms[WG / 64][2048];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * (WG / 64) + wave;
    if (c > k) return;   // (c == k: the trailing bucket of ids outside [0, k); sorted too when it fits)
    const uint32_t beg = offsets[c], len = offsets[c + 1] - beg;
    if (len < 2 || len > long_list || len > 2048u) return;
    uint32_t P = 2;
    while (P < len) P <<= 1;
    uint32_t* s = ms[wave];
    for (uint32_t i = lane; i < P; i += 64) s[i] = i < len ? order[beg + i] : 0xffffffffu;
    for (uint32_t size = 2; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __builtin_amdgcn_wave_barrier();   // (a wave's LDS operations execute in order; this keeps the compiler from moving them)
            for (uint32_t i = lane; i < P / 2; i += 64) {
                const uint32_t pos = 2 * i - (i & (stride - 1));
                const uint32_t a = s[pos], b = s[pos + stride];
                const bool up = (pos & size) == 0;
                if ((a > b) == up) { s[pos] = b; s[pos + stride] = a; }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = lane; i < len; i += 64) order[beg + i] = s[i];
}

// the few long clusters beyond the compaction's EARLY_MAX: rank sort of the scattered segment by one workgroup
// (rows are distinct: rank = number of smaller rows), through a scratch copy
__global__ void __launch_bounds__(1024) long_ranksort_kernel(uint32_t* __restrict__ order, const uint32_t* __restrict__ offsets,
                                                             const int* __restrict__ longs, uint32_t* __restrict__ scratch) {
    __shared__ uint32_t tile[1024];
    const int nl = longs[0];
    for (int slot = EARLY_MAX + blockIdx.x; slot < nl; slot += gridDim.x) {
        const int c = longs[1 + slot];
        const uint32_t beg = offsets[c], len = offsets[c + 1] - beg;
        for (uint32_t i0 = 0; i0 < len; i0 += 1024) {
            const uint32_t i = i0 + threadIdx.x;
            const uint32_t mine = i < len ? order[beg + i] : 0u;
            uint32_t rank = 0;
            for (uint32_t j0 = 0; j0 < len; j0 += 1024) {
                __syncthreads();
                tile[threadIdx.x] = j0 + threadIdx.x < len ? order[beg + j0 + threadIdx.x] : 0xffffffffu;
                __syncthreads();
                const uint32_t m = min(1024u, len - j0);
                for (uint32_t j = 0; j < m; j++) rank += tile[j] < mine;
            }
            if (i < len) scratch[beg + rank] = mine;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < len; i += 1024) order[beg + i] = scratch[beg + i];
        __syncthreads();
    }
}

// sorted_ids[p] = the cluster of position p (k for the trailing bucket of invalid ids)
// (and, when the caller wants the member order too, its copy out of the workspace in the same pass)
__global__ void __launch_bounds__(WG) segment_ids_kernel(const uint32_t* __restrict__ offsets, int k, uint32_t* __restrict__ sorted_ids,
                                                         const uint32_t* __restrict__ order, uint32_t* __restrict__ order_out) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (c > k) return;
    for (uint32_t p = offsets[c] + lane; p < offsets[c + 1]; p += 64) {
        sorted_ids[p] = (uint32_t)c;
        if (order_out) order_out[p] = order[p];
    }
}

// ---- host driver ------------------------------------------------------------------------------------------------
// One call: its arguments, and everything that is decided about it -- from (n, d, k, the alignment of x, the switch
// accum_buckets) alone, before anything is queued.  Every launch below reads the plan.
struct AccumPlan {
    const float* x; const long* ids; long n; int d, k; float *sums, *counts; hipStream_t stream;   // the call
    bool use_buckets;      // member lists by counting and scattering, else by radix sort
    uint32_t long_list;    // member lists longer than this go to the feature-sliced kernel (without it every list is a short one)
    bool have_long;        // some list may be that long: the side stream gets work
    bool offsets_beside;   // sort strategy: the segment offsets come from a count + scan beside the sort
    int vec, slabs;        // the short-list kernel: features per lane, 64 * vec-feature slabs per row
    unsigned grid;
    int rows_per_block, count_blocks;   // the count / scatter passes over ids
    size_t count_lds;
    int nblk;              // row blocks of the ordered compaction
};

AccumPlan accum_plan(const at_ctx* ctx, const float* x, int64_t n, int d, const int64_t* ids, int k, float* sums, float* counts,
                     hipStream_t stream) {
    AccumPlan p{x, reinterpret_cast<const long*>(ids), (long)n, d, k, sums, counts, stream};
    const bool al = at_aligned16(x), long_ok = d % 4 == 0 && al;
    p.long_list = long_ok ? AccumShape<false>::LONG_LIST : UINT32_MAX;
    // The long lists are one dependent add chain per feature (the contract's summation order), a few
    // workgroups busy for as long as the longest list takes: they run on a side stream beside the
    // kernel that handles all the other clusters.
    p.have_long = long_ok && n > (int64_t)p.long_list;
    // The bucket path pays off where the radix sort's eight launches are fixed cost: few rows per cluster (the
    // per-rank share of a sharded run).  At 2 M rows its scattered 4-byte stores (134 us) and the in-LDS order of 1000+
    // row lists (159 us) lose to two onesweep passes.  (It hands lists longer than 2048 rows to the feature-sliced
    // kernel: that needs d % 4 == 0.)
    p.use_buckets = ctx->dbg.accum_buckets != 0 && k <= 16384 && n <= 64 * (int64_t)k && long_ok;
    // The segment offsets do not need the sort: counts per cluster (LDS histogram per row block) and their scan
    // -- the first two kernels of the bucket path -- run beside it, instead of 8193 binary searches over the
    // sorted keys behind it (40 us on the critical path of a 2 M-row iteration).
    p.offsets_beside = !p.use_buckets && p.have_long && k <= 16384;
    p.vec = d % 4 == 0 && d >= 256 && al ? 4 : d % 2 == 0 && d >= 128 && al ? 2 : 1;
    p.slabs = (d + 64 * p.vec - 1) / (64 * p.vec);
    p.grid = (unsigned)(((long)k * p.slabs + WG / 64 - 1) / (WG / 64));
    // rows per workgroup of the count / scatter passes: enough workgroups to fill the chip at small n (each pays
    // three passes over the k bins), 4096 rows at large n
    const int rpb = (int)(n / 1024);
    p.rows_per_block = ((rpb < 512 ? 512 : (rpb > 4096 ? 4096 : rpb)) + WG - 1) / WG * WG;
    p.count_blocks = (int)((n + p.rows_per_block - 1) / p.rows_per_block);
    p.count_lds = ((size_t)k + 1) * 4;
    p.nblk = (int)((n + EARLY_ROWS - 1) / EARLY_ROWS);
    return p;
}

// The side stream's share of one call.  Every return of at_centroid_accum_f32 goes through finish().
struct SideWork {
    at_ctx* ctx;
    hipStream_t stream;   // the caller's
    bool begun = false, joined = false;
    // the side stream waits for what `stream` has queued so far
    int begin() {
        if (!ctx->side_stream) AT_HIP(hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
        for (hipEvent_t* ev : {&ctx->side_ev[0], &ctx->side_ev[1], &ctx->side_ev2})
            if (!*ev) AT_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
        AT_HIP(hipEventRecord(ctx->side_ev[0], stream));
        AT_HIP(hipStreamWaitEvent(ctx->side_stream, ctx->side_ev[0], 0));
        begun = true;
        return AT_OK;
    }
    int end() { AT_HIP(hipEventRecord(ctx->side_ev[1], ctx->side_stream)); return AT_OK; }   // it has all of its work
    int join() { AT_HIP(hipStreamWaitEvent(stream, ctx->side_ev[1], 0)); joined = true; return AT_OK; }   // `stream` waits for it
    // The caller's stream must not read `sums` before the side stream is done.  Under the "deferred" protocol
    // (at_centroid_accum_defer) the wait is left to the caller's at_centroid_accum_join, who can queue independent
    // work (the next iteration's visiting order) behind the short-list kernel meanwhile.  A failed call never defers:
    // `stream` waits for whatever the side stream was given, so the caller may free x / ids / sums behind it.
    int finish(int rc) {
        if (!begun || joined) return rc;
        if (rc == AT_OK && !ctx->defer_join) return join();
        if (rc == AT_OK) ctx->join_pending = 1;
        else if (AT_HIP_TOLERATE(hipEventRecord(ctx->side_ev[1], ctx->side_stream)) == hipSuccess)
            (void)AT_HIP_TOLERATE(hipStreamWaitEvent(stream, ctx->side_ev[1], 0));
        return rc;
    }
};

// The member lists of up to EARLY_MAX clusters (pred[0 .. *pred_n)) by ordered compaction of ids: list m at el.eoff[m]
// of `lists`, or -- seg_offsets given -- in the cluster's own segment of `lists`.
int queue_early_lists(hipStream_t ss, const AccumPlan& p, const int* pred, const int* pred_n, const EarlyLists& el,
                      uint32_t* lists, const uint32_t* seg_offsets) {
    AT_LAUNCH(early_count_kernel, dim3(p.nblk), dim3(WG), 0, ss, p.ids, p.n, pred, pred_n, p.nblk, el.blockcnt);
    AT_LAUNCH(early_scan_kernel, dim3(1), dim3(1024), 0, ss, el.blockcnt, p.nblk, el.blockbase, el.eoff);
    AT_LAUNCH(early_write_kernel, dim3(p.nblk), dim3(WG), 0, ss, p.ids, p.n, pred, pred_n, p.nblk, el.blockbase,
              seg_offsets ? nullptr : el.eoff, lists, seg_offsets);
    return AT_OK;
}

int launch_short_lists(const AccumPlan& p, const uint32_t* order, const uint32_t* offsets) {
    auto* centroid_accum_kernel_vec = p.vec == 4 ? centroid_accum_kernel<4, false> : p.vec == 2 ? centroid_accum_kernel<2, false> : centroid_accum_kernel<1, false>;
    AT_LAUNCH(centroid_accum_kernel_vec, dim3(p.grid), dim3(WG), 0, p.stream, p.x, nullptr, p.d, order, offsets, p.k, p.slabs, p.long_list,
              p.sums, p.counts);
    return AT_OK;
}

// What a strategy leaves (the long clusters' sums queued on the side stream): members order[offsets[c] .. offsets[c + 1]) in
// ascending row order; sorted_keys: the cluster of every position, where the strategy has it.
struct MemberLists { const uint32_t *order, *offsets, *sorted_keys; };

// k <= 16 384: see "member lists without a radix sort" above.
int lists_by_buckets(at_ctx* ctx, const AccumPlan& p, SideWork& side, MemberLists* out) {
    const size_t nn = (size_t)(p.n > 0 ? p.n : 1);
    uint32_t* order = static_cast<uint32_t*>(at_ws(ctx, WS_SORT_VALS_A, nn * 4, p.stream));
    uint32_t* offsets = static_cast<uint32_t*>(at_ws(ctx, WS_SEG_OFFSETS, ((size_t)p.k + 2) * 4, p.stream));
    if (!order || !offsets) return AT_E_NOMEM;
    BucketTable bt;
    EarlyLists el;
    AT_TRY(bt.fetch(ctx, p.k, p.stream));
    AT_TRY(el.fetch(ctx, p.nblk, nn, p.stream));
    AT_RAISE_LDS(ctx, bucket_count_kernel, p.count_lds);
    AT_RAISE_LDS(ctx, bucket_scatter_kernel, 2 * p.count_lds);
    *out = MemberLists{order, offsets, nullptr};
    hipStream_t ss = nullptr;
    if (p.n > 0)
        AT_LAUNCH(bucket_count_kernel, dim3(p.count_blocks), dim3(WG), p.count_lds, p.stream, p.ids, p.n, p.k, p.rows_per_block, bt.counts);
    AT_LAUNCH(bucket_scan_kernel, dim3(1), dim3(1024), 0, p.stream, bt.counts, p.k, p.long_list, offsets, bt.cursor, bt.longs);
    if (p.have_long) {
        // side stream: the long clusters' members by ordered compaction straight into their segments, then their sums
        AT_TRY(side.begin());   // offsets / longs are ready
        ss = ctx->side_stream;
        AT_TRY(queue_early_lists(ss, p, bt.longs + 1, bt.longs, el, order, offsets));
        AT_LAUNCH(centroid_accum_long_kernel<false>, dim3(EARLY_MAX, p.d / 4), dim3(WG), 0, ss, p.x, nullptr, p.d, order, offsets, p.long_list,
                  p.sums, p.counts, p.k, 0, bt.longs, nullptr, nullptr, 0u, 0, EARLY_MAX);
    }
    if (p.n > 0) {
        AT_LAUNCH(bucket_scatter_kernel, dim3(p.count_blocks), dim3(WG), 2 * p.count_lds, p.stream, p.ids, p.n, p.k, p.rows_per_block,
                  bt.cursor, order);
        // (lists of 1025 .. 2048 rows that no local sort took: none, member_sort_kernel's capacity is 2048)
        AT_LAUNCH(member_sort_kernel, dim3((p.k + 1 + WG / 64 - 1) / (WG / 64)), dim3(WG), 0, p.stream, order, offsets, p.k, 2048u);
    }
    if (p.have_long) {
        // more than EARLY_MAX long clusters (rare): the rest were scattered; rank-sort them, then their sums
        AT_TRY(side.begin());   // scattered segments are ready
        AT_LAUNCH(long_ranksort_kernel, dim3(16), dim3(1024), 0, ss, order, offsets, bt.longs, el.lists);
        AT_LAUNCH(centroid_accum_long_kernel<false>, dim3(16, p.d / 4), dim3(WG), 0, ss, p.x, nullptr, p.d, order, offsets, p.long_list,
                  p.sums, p.counts, p.k, 0, bt.longs, nullptr, nullptr, 0u, EARLY_MAX, 0x7fffffff);
        AT_TRY(side.end());
    }
    return AT_OK;
}

// Any k: a stable radix sort of (cluster, row) pairs.  The clusters that were long in the previous call get their
// lists and sums on the side stream beside the sort, the other long ones behind it.
int lists_by_sort(at_ctx* ctx, const AccumPlan& p, SideWork& side, MemberLists* out) {
    const size_t nn = (size_t)(p.n > 0 ? p.n : 1);
    uint32_t* keys_a = static_cast<uint32_t*>(at_ws(ctx, WS_SORT_KEYS_A, nn * 4, p.stream));
    uint32_t* keys_b = static_cast<uint32_t*>(at_ws(ctx, WS_SORT_KEYS_B, nn * 4, p.stream));
    uint32_t* vals_a = static_cast<uint32_t*>(at_ws(ctx, WS_SORT_VALS_A, nn * 4, p.stream));
    uint32_t* vals_b = static_cast<uint32_t*>(at_ws(ctx, WS_SORT_VALS_B, nn * 4, p.stream));
    uint32_t* offsets = static_cast<uint32_t*>(at_ws(ctx, WS_SEG_OFFSETS, ((size_t)p.k + 2) * 4, p.stream));
    if (!keys_a || !keys_b || !vals_a || !vals_b || !offsets) return AT_E_NOMEM;
    LongPred lp;
    EarlyLists el;
    int* late = nullptr;
    unsigned gen = 0;
    hipStream_t ss = nullptr;
    if (p.have_long) {
        AT_TRY(lp.fetch(ctx, p.k, p.stream));
        AT_TRY(el.fetch(ctx, p.nblk, nn, p.stream));
        late = static_cast<int*>(at_ws(ctx, WS_LONG_LATE, ((size_t)p.k + 1) * 4, p.stream));
        if (!late) return AT_E_NOMEM;
        gen = ++ctx->long_gen;   // (the early pass and the pass behind the sort take the same generation)
        AT_TRY(side.begin());    // ids (and the marks) are ready
        ss = ctx->side_stream;
        if (p.offsets_beside) {
            BucketTable bt;
            AT_TRY(bt.fetch(ctx, p.k, ss));
            AT_RAISE_LDS(ctx, bucket_count_kernel, p.count_lds);
            AT_LAUNCH(bucket_count_kernel, dim3(p.count_blocks), dim3(WG), p.count_lds, ss, p.ids, p.n, p.k, p.rows_per_block, bt.counts);
            AT_LAUNCH(bucket_scan_kernel, dim3(1), dim3(1024), 0, ss, bt.counts, p.k, p.long_list, offsets, bt.cursor, bt.longs);
            AT_HIP(hipEventRecord(ctx->side_ev2, ss));
        }
        AT_TRY(queue_early_lists(ss, p, lp.pred, lp.pred_n, el, el.lists, nullptr));
        AT_LAUNCH(centroid_accum_long_kernel<false>, dim3(EARLY_MAX, p.d / 4), dim3(WG), 0, ss, p.x, nullptr, p.d, el.lists, el.eoff, p.long_list,
                  p.sums, p.counts, p.k, 1, lp.pred, lp.pred_n, lp.done, gen, 0, 0x7fffffff);
        // the regular pass rebuilds the prediction: its counter starts from zero once the early pass has read it
        AT_HIP(hipMemsetAsync(lp.pred_n, 0, 4, ss));
    }
    *out = MemberLists{vals_a, offsets, keys_a};
    if (p.n > 0) {
        AT_LAUNCH(make_keys_kernel, dim3((unsigned)((p.n + WG - 1) / WG)), dim3(WG), 0, p.stream, p.ids, p.n, p.k, keys_a, vals_a);
        unsigned bits = 1;
        while ((1u << bits) <= (unsigned)p.k) bits++;  // keys take values 0..k
        rocprim::double_buffer<uint32_t> kb(keys_a, keys_b);
        rocprim::double_buffer<uint32_t> vb(vals_a, vals_b);
        AT_TRY(at_sort_pairs(ctx, WS_SORT_TMP, kb, vb, (size_t)p.n, 0, bits, p.stream));
        *out = MemberLists{vb.current(), offsets, kb.current()};
    }
    if (p.offsets_beside)
        AT_HIP(hipStreamWaitEvent(p.stream, ctx->side_ev2, 0));
    else
        AT_LAUNCH(segment_offsets_kernel, dim3((p.k + 1 + WG - 1) / WG), dim3(WG), 0, p.stream, out->sorted_keys, p.n, p.k, p.long_list, offsets, nullptr);
    if (p.have_long) {
        AT_TRY(side.begin());   // sorted lists and offsets are ready
        AT_HIP(hipMemsetAsync(late, 0, 4, ss));
        AT_LAUNCH(long_detect_kernel, dim3((p.k + WG - 1) / WG), dim3(WG), 0, ss, offsets, p.k, p.long_list, lp.done, gen, lp.pred,
                  lp.pred_n, late);
        AT_LAUNCH(centroid_accum_long_kernel<false>, dim3(32, p.d / 4), dim3(WG), 0, ss, p.x, nullptr, p.d, out->order, offsets, p.long_list,
                  p.sums, p.counts, p.k, 0, late, nullptr, lp.done, gen, 0, 0x7fffffff);
        AT_TRY(side.end());
    }
    return AT_OK;
}

int accum_queue(at_ctx* ctx, const AccumPlan& p, uint32_t* order_out, uint32_t* sorted_ids_out, SideWork& side) {
    MemberLists m;
    AT_TRY(p.use_buckets ? lists_by_buckets(ctx, p, side, &m) : lists_by_sort(ctx, p, side, &m));
    AT_TRY(launch_short_lists(p, m.order, m.offsets));   // (when the sliced kernel cannot run, lists of any length)
    if (p.n == 0 || !(order_out || sorted_ids_out)) return AT_OK;
    const size_t bytes = sizeof(uint32_t) * (size_t)p.n;
    if (m.sorted_keys) {
        if (order_out) AT_HIP(hipMemcpyAsync(order_out, m.order, bytes, hipMemcpyDeviceToDevice, p.stream));
        if (sorted_ids_out) AT_HIP(hipMemcpyAsync(sorted_ids_out, m.sorted_keys, bytes, hipMemcpyDeviceToDevice, p.stream));
        return AT_OK;
    }
    // Bucket strategy: a caller that wants the member order gets the long clusters' segments too, and those are written
    // on the side stream: its work is waited for BEFORE the order leaves the workspace.
    if (p.have_long) AT_TRY(side.join());
    if (sorted_ids_out)   // (the segments [offsets[0], offsets[k+1]) cover every position: the copy of the order rides along)
        AT_LAUNCH(segment_ids_kernel, dim3((p.k + 1 + WG / 64 - 1) / (WG / 64)), dim3(WG), 0, p.stream, m.offsets, p.k, sorted_ids_out,
                  m.order, order_out);
    else
        AT_HIP(hipMemcpyAsync(order_out, m.order, bytes, hipMemcpyDeviceToDevice, p.stream));
    return AT_OK;
}

}  // namespace

extern "C" {

int at_centroid_accum_f32(at_ctx* ctx, const float* x, int64_t n, int d, const int64_t* ids, int k, float* sums, float* counts,
                          uint32_t* order_out, uint32_t* sorted_ids_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx, "at_centroid_accum_f32: ctx is null");
    AT_REQUIRE(n >= 0 && n < (int64_t)UINT32_MAX && d > 0 && k > 0 && k < (1 << 30),
               "at_centroid_accum_f32: bad sizes n=%lld d=%d k=%d", (long long)n, d, k);
    AT_REQUIRE(sums && counts && (n == 0 || (x && ids)), "at_centroid_accum_f32: null pointer");
    AT_HIP(hipSetDevice(ctx->device));
    const AccumPlan p = accum_plan(ctx, x, n, d, ids, k, sums, counts, stream);
    SideWork side{ctx, stream};
    return side.finish(accum_queue(ctx, p, order_out, sorted_ids_out, side));
}

// at_centroid_accum_defer(ctx, 1): following at_centroid_accum_f32 calls return without making `stream` wait
// for the long-list kernel on the context's side stream; at_centroid_accum_join(ctx, stream) inserts that
// wait (a no-op when nothing is pending) and must precede any use of the sums / counts.
int at_centroid_accum_defer(at_ctx* ctx, int on) {
    AT_REQUIRE(ctx, "at_centroid_accum_defer: ctx is null");
    ctx->defer_join = on ? 1 : 0;
    return AT_OK;
}

int at_centroid_accum_join(at_ctx* ctx, void* stream_) {
    AT_REQUIRE(ctx, "at_centroid_accum_join: ctx is null");
    if (!ctx->join_pending) return AT_OK;
    AT_HIP(hipSetDevice(ctx->device));
    AT_HIP(hipStreamWaitEvent((hipStream_t)stream_, ctx->side_ev[1], 0));
    ctx->join_pending = 0;
    return AT_OK;
}

}  // extern "C"
