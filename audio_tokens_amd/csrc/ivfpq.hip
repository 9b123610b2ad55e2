// ivfpq.hip -- product-quantiser codes behind inverted lists on gfx950: at_ivfpq_build, at_ivfpq_search_f32
// (ops.IndexIVFPQ).  Contract: include/audio_tokens_amd.h, DESIGN.md section 6p -- the library's own, in the manner of
// faiss.IndexIVFPQ under L2, recalled, not verified against faiss output.
//
// Arithmetic: for query i and probed list l the query vector is q = x[i] - c[l], one fp32 subtraction per feature
// (by_residual), or x[i] itself.  The table is T[m][j] = sum_f (q[m * dsub + f] - cb[m][j][f])^2 in pq_search.hip's direct
// form -- df one subtraction, acc = fmaf(df, df, acc) from +0 over ascending f -- and a stored row r of list l has
// dis = T[0][code[r][0]] + T[1][code[r][1]] + ..., one fp32 addition per step in ascending m.  q is recomputed per table
// entry, which gives the bits of staging it once.  The expansion form appears nowhere, and neither does faiss's
// precomputed-table decomposition of the residual distance.
//
// The image (at_ivfpq_build): the code rows grouped by list in ascending id (the caller's stable order), every list
// padded to whole groups of GROUP = 16 rows, so a list starts 16-byte aligned for any M and pq_scan_kernel's 16-, 8-, 4-
// and 1-byte loads apply unchanged.  pos2id[position] is the id of the row at a position, -1 for a pad; first[l] is the
// first group of list l, first[nlist] the number of groups in use.
//
// The search (at_ivfpq_search_f32), per chunk of queries, all on the stream: pair_inversion.h's counting sort of the
// (query, probe) pairs by list in blocks of QB pairs (pq_keys.h: 4 for M <= 32, 2 above); the scan -- one workgroup per
// (list, block of QB probing pairs), found by binary search in blk_start, builds the QB tables of its pairs with the
// pairs innermost, lut[m][j][q], walks the positions [first[l] * 16, first[l + 1] * 16) in rounds of 256 rows with
// pq_scan_kernel's look-up loop and candidate buffer (pq_keys.h; the QB buffers of a workgroup go through the sorting
// network together, sort_keys_all below), and writes k keys (distance bits << 32) | id per pair;
// the merge -- pq_keys.h's pq_merge_kernel, one workgroup per query streaming its nprobe * k keys: ivf.hip's merge makes
// k passes over them, which at k = 128 is 128 times the reads.  A list of any length is walked by the workgroups of its
// own pair blocks alone: very long lists are not split into slabs.
//
// Every index that addresses memory is derived from tables this file builds, and is compared with the host-side bound
// of the array it addresses before it is used: a torn table may lose results, it cannot address out of range.
#include "at_internal.h"
#include "pair_inversion.h"
#include "pq_keys.h"

namespace {

using namespace pqk;
using pinv::ivf_count_kernel;
using pinv::ivf_offsets_kernel;
using pinv::ivf_scatter_kernel;
using pinv::list_of_unit;

constexpr int GROUP = 16;            // rows a list is padded to: GROUP * M bytes are a multiple of 16 for any M
constexpr int MAX_NLIST = 1 << 24;
constexpr size_t BUDGET_BYTES = (size_t)256 << 20;   // the partial lists of one chunk of queries
constexpr int64_t MAX_PAIRS = (int64_t)1 << 30;      // (query, probe) pairs of one chunk: pair indices are ints
constexpr int64_t MAX_CHUNK = ((int64_t)1 << 24) - 4;   // the merge is a workgroup per query: chunk * WG work-items < 2^32

int64_t queries_per_chunk(int nprobe, int k) {
    int64_t chunk = (int64_t)(BUDGET_BYTES / (sizeof(uint64_t) * (size_t)nprobe * k));
    if (chunk > MAX_PAIRS / nprobe) chunk = MAX_PAIRS / nprobe;
    if (chunk > MAX_CHUNK) chunk = MAX_CHUNK;
    return chunk < 1 ? 1 : chunk;
}

// one thread per position of the grouped image
__global__ void __launch_bounds__(WG)
ivfpq_group_kernel(const uint8_t* __restrict__ codes, const long* __restrict__ lists, const long* __restrict__ order,
                   long ntotal, int M, int nlist, const int* __restrict__ start, const int* __restrict__ first,
                   int ngroups, uint8_t* __restrict__ out, int* __restrict__ pos2id) {
    const long pos = (long)blockIdx.x * WG + threadIdx.x;
    if (pos >= (long)ngroups * GROUP) return;
    const int g = (int)(pos / GROUP);
    long id = -1;
    // a group behind the last list (the host's bound is not tight) is all pads and never read
    if (g < first[nlist]) {
        const int l = list_of_unit(first, nlist, g);
        const long at = (long)(g - first[l]) * GROUP + pos % GROUP;
        const long p = (long)start[l] + at;
        // p < start[l + 1] <= ntotal by the prefix sum; the row it names must be one of list l, or `order` is not what
        // the contract asks for and the position stays a pad
        if (at < (long)start[l + 1] - start[l] && p >= 0 && p < ntotal) {
            id = order[p];
            if (id < 0 || id >= ntotal || lists[id] != l) id = -1;
        }
    }
    pos2id[pos] = (int)id;
    uint8_t* o = out + pos * M;
    for (int m = 0; m < M; m++) o[m] = id >= 0 ? codes[id * M + m] : (uint8_t)0;
}

// pq_keys.h's sort_keys over the QB buffers of a workgroup in one pass of the network: buffer q sorts its first cnt[q]
// places (0: it is left alone), the places from there up to the power of two above the largest count again counting as
// all-ones keys, and one barrier per step serves all the buffers.  A workgroup here walks a list of a few thousand rows,
// not a slab of 65 536, so its sorts are a large share of its time.  cnt is the same in every thread.  Ends behind a
// barrier.
template <int QB>
__device__ void sort_keys_all(uint64_t* buf, const int (&cnt)[QB]) {
    const int t = threadIdx.x;
    int top = 0;
#pragma unroll
    for (int q = 0; q < QB; q++) top = cnt[q] > top ? cnt[q] : top;
    int P = 2;
    while (P < top) P <<= 1;
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int i = 2 * t - (t & (stride - 1));
            const int j = 2 * stride == size ? (i | (size - 1)) - (i & (stride - 1)) : i + stride;
#pragma unroll
            for (int q = 0; q < QB; q++)
                if (j < cnt[q]) {   // (i < j)
                    uint64_t* bq = buf + q * CAP;
                    const uint64_t a = bq[i], b = bq[j];
                    if (a > b) {
                        bq[i] = b;
                        bq[j] = a;
                    }
                }
            __syncthreads();
        }
}

// QB pairs per workgroup, code rows in pieces of W bytes (M % W == 0, the image W-byte aligned), FULL: ksub == 256,
// RESID: the query of a pair is x - centroid of the list
template <int QB, int W, bool FULL, bool RESID>
__global__ void __launch_bounds__(WG)
ivfpq_scan_kernel(const float* __restrict__ x, int d, int M, int ksub, const float* __restrict__ cb,
                  const float* __restrict__ cent, int nprobe, int ptotal, int nlist, const int* __restrict__ pair_start,
                  const int* __restrict__ blk_start, const int* __restrict__ pairtab, const uint8_t* __restrict__ codes,
                  const int* __restrict__ first, int ngroups, const int* __restrict__ pos2id, long ntotal, int k,
                  uint64_t* __restrict__ partial) {
    typedef float fq __attribute__((ext_vector_type(QB)));
    typedef typename Piece<W>::type piece_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // The grid is the host's bound; the workgroups behind the real count leave as a whole, before the first barrier.
    // Everything up to the table build is the same in every thread of the workgroup.
    const int b = blockIdx.x;
    if (b >= blk_start[nlist]) return;
    const int l = list_of_unit(blk_start, nlist, b);
    // blk_start[l] <= b < blk_start[l + 1] = blk_start[l] + ceil(c / QB), c the pairs of list l:
    // (b - blk_start[l]) * QB < c, so the block holds 1 .. QB pairs, all inside the list's stretch of pairtab
    const int p0 = pair_start[l] + (b - blk_start[l]) * QB;
    int cnt = pair_start[l + 1] - p0;
    if (cnt > QB) cnt = QB;
    if (cnt < 1 || p0 < 0 || p0 + cnt > ptotal) return;
    // first ascends and first[nlist] <= ngroups (the host's bound on the groups of the image)
    int g0 = first[l], g1 = first[l + 1];
    if (g0 < 0) g0 = 0;
    if (g1 > ngroups) g1 = ngroups;
    const long s0 = (long)g0 * GROUP, s1 = (long)g1 * GROUP;

    const int tid = threadIdx.x;
    int pair[QB];
    bool valid[QB];
    const float* xq[QB];
#pragma unroll
    for (int q = 0; q < QB; q++) {
        // a slot behind the block's count computes the block's first pair again and stores nothing
        valid[q] = q < cnt;
        pair[q] = pairtab[p0 + (valid[q] ? q : 0)];
        if (pair[q] < 0 || pair[q] >= ptotal) {   // pairtab holds pair indices < ptotal only (ivf_scatter_kernel)
            pair[q] = 0;
            valid[q] = false;
        }
        xq[q] = x + (size_t)(pair[q] / nprobe) * d;   // pair / nprobe < ptotal / nprobe = the chunk's queries
    }
    if (s1 <= s0) {   // an empty list: no table is worth building
#pragma unroll
        for (int q = 0; q < QB; q++)
            if (valid[q])
                for (int t = tid; t < k; t += WG) partial[(size_t)pair[q] * k + t] = KEY_NONE;
        return;
    }

    const int entries = M * ksub;
    fq* lut = reinterpret_cast<fq*>(smem);                                           // [M][ksub][QB]
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem + sizeof(float) * QB * (size_t)entries);   // [QB][CAP]
    auto counters = [&](int q) { return reinterpret_cast<int*>(buf + q * CAP + CAP - 2); };   // three words per query
    const int dsub = d / M;
    const float* cl = RESID ? cent + (size_t)l * d : nullptr;   // l < nlist: list_of_unit

    // ksub <= WG: thread j owns word j of every sub-space, so the sub-vector of a pair is the same address in every
    // thread and the codebook word is read once for all QB pairs
    for (int m = 0; m < M; m++) {
        if (tid < ksub) {
            const int e = m * ksub + tid;
            const float* c = cb + (size_t)e * dsub;
            float acc[QB];
#pragma unroll
            for (int q = 0; q < QB; q++) acc[q] = 0.0f;
            for (int f = 0; f < dsub; f++) {
                const float cf = c[f];
#pragma unroll
                for (int q = 0; q < QB; q++) {
                    float qv = xq[q][m * dsub + f];
                    if constexpr (RESID) qv = qv - cl[m * dsub + f];
                    const float df = qv - cf;
                    acc[q] = __builtin_fmaf(df, df, acc[q]);
                }
            }
            fq v;
#pragma unroll
            for (int q = 0; q < QB; q++) v[q] = acc[q];
            lut[e] = v;
        }
    }
    if (tid < 3 * QB) counters(tid / 3)[tid % 3] = 0;
    __syncthreads();

    const int npieces = M / W;
    int base[QB];
    uint64_t thr[QB];   // the same in every thread
#pragma unroll
    for (int q = 0; q < QB; q++) {
        base[q] = 0;
        thr[q] = KEY_LIMIT;
    }
    int cur = 0;

    // rows are positions of the image: s1 <= ngroups * GROUP, the length of pos2id and (times M) of codes
    piece_t v = piece_t();
    if (s0 + tid < s1) v = *reinterpret_cast<const piece_t*>(codes + (s0 + tid) * (long)M);
    for (long r0 = s0; r0 < s1; r0 += WG) {
        const long row = r0 + tid;
        const bool inside = row < s1;
        long id = -1;
        if (inside) id = pos2id[row];
        bool listed = id >= 0 && id < ntotal;   // a pad or an id out of range is dropped
        fq acc;
#pragma unroll
        for (int q = 0; q < QB; q++) acc[q] = 0.0f;
        for (int p = 0; p < npieces; p++) {
            piece_t nx = piece_t();
            if (p + 1 < npieces) {
                if (inside) nx = *reinterpret_cast<const piece_t*>(codes + row * (long)M + (p + 1) * W);
            } else if (row + WG < s1) {
                nx = *reinterpret_cast<const piece_t*>(codes + (row + WG) * (long)M);
            }
#pragma unroll
            for (int bb = 0; bb < W; bb++) {
                unsigned code = piece_byte<W>(v, bb);
                const int m = p * W + bb;
                if constexpr (FULL) {
                    acc += lut[(m << 8) | code];
                } else {
                    if (code >= (unsigned)ksub) {
                        listed = false;
                        code = ksub - 1;
                    }
                    acc += lut[m * ksub + code];
                }
            }
            v = nx;
        }

        const int nxt = cur == 2 ? 0 : cur + 1;
        if (tid < QB) counters(tid)[nxt] = 0;
        if (listed) {
#pragma unroll
            for (int q = 0; q < QB; q++) {
                const uint64_t key = ((uint64_t)__float_as_uint(acc[q]) << 32) | (uint32_t)id;
                if (key < thr[q]) {
                    const int s = base[q] + atomicAdd(counters(q) + cur, 1);
                    buf[q * CAP + s] = key;
                }
            }
        }
        __syncthreads();
        // cut_to_k for every buffer a round could overflow, in one pass: FULL_AT >= MAX_K, so such a buffer holds k keys
        int full[QB];
        bool any = false;
#pragma unroll
        for (int q = 0; q < QB; q++) {
            base[q] += counters(q)[cur];
            full[q] = base[q] > FULL_AT ? base[q] : 0;
            any |= full[q] > 0;
        }
        if (any) {
            sort_keys_all<QB>(buf, full);
#pragma unroll
            for (int q = 0; q < QB; q++)
                if (full[q] >= k) {   // (every thread reads the threshold for itself: the appends that follow go behind it)
                    thr[q] = buf[q * CAP + k - 1];
                    base[q] = k;
                }
        }
        cur = nxt;
    }

    sort_keys_all<QB>(buf, base);
#pragma unroll
    for (int q = 0; q < QB; q++) {
        const int kept = base[q] < k ? base[q] : k;
        if (valid[q]) {
            uint64_t* out = partial + (size_t)pair[q] * k;
            for (int t = tid; t < k; t += WG) out[t] = t < kept ? buf[q * CAP + t] : KEY_NONE;
        }
    }
}

size_t scan_lds_bytes(int qb, int M, int ksub) {
    return sizeof(float) * qb * (size_t)M * ksub + sizeof(uint64_t) * qb * CAP;
}

struct ScanArgs {
    const float* x;
    int d, M, ksub;
    const float* cb;
    const float* cent;
    int nprobe, ptotal, nlist;
    const int *pair_start, *blk_start, *pairtab;
    const uint8_t* codes;
    const int* first;
    int ngroups;
    const int* pos2id;
    int64_t ntotal;
    int k;
    uint64_t* partial;
};

template <int QB, int W, bool FULL, bool RESID>
int launch_scan(at_ctx* ctx, const ScanArgs& a, hipStream_t stream) {
    const size_t lds = scan_lds_bytes(QB, a.M, a.ksub);
    // sum over the lists of ceil(c / QB) <= ptotal / QB + the number of probed lists
    const unsigned grid = (unsigned)(a.ptotal / QB + (a.nlist < a.ptotal ? a.nlist : a.ptotal));
    AT_RAISE_LDS(ctx, (ivfpq_scan_kernel<QB, W, FULL, RESID>), lds);
    AT_LAUNCH((ivfpq_scan_kernel<QB, W, FULL, RESID>), dim3(grid), dim3(WG), lds, stream, a.x, a.d, a.M, a.ksub, a.cb,
              a.cent, a.nprobe, a.ptotal, a.nlist, a.pair_start, a.blk_start, a.pairtab, a.codes, a.first, a.ngroups,
              a.pos2id, (long)a.ntotal, a.k, a.partial);
    return AT_OK;
}

template <int QB, int W>
int launch_scan_by_form(at_ctx* ctx, const ScanArgs& a, hipStream_t stream) {
    if (a.ksub == 256) return a.cent ? launch_scan<QB, W, true, true>(ctx, a, stream) : launch_scan<QB, W, true, false>(ctx, a, stream);
    return a.cent ? launch_scan<QB, W, false, true>(ctx, a, stream) : launch_scan<QB, W, false, false>(ctx, a, stream);
}

template <int QB>
int launch_scan_by_width(at_ctx* ctx, const ScanArgs& a, hipStream_t stream) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a.codes);
    if (a.M % 16 == 0 && p % 16 == 0) return launch_scan_by_form<QB, 16>(ctx, a, stream);
    if (a.M % 8 == 0 && p % 8 == 0) return launch_scan_by_form<QB, 8>(ctx, a, stream);
    if (a.M % 4 == 0 && p % 4 == 0) return launch_scan_by_form<QB, 4>(ctx, a, stream);
    return launch_scan_by_form<QB, 1>(ctx, a, stream);
}

size_t ws_align(size_t b) { return (b + 255) & ~size_t(255); }

}  // namespace

extern "C" int at_ivfpq_search_limits(int* pairs_per_block, int* rows_per_group, int64_t* queries_per_chunk_out, int M,
                                      int nprobe, int k) {
    AT_REQUIRE(M >= 1 && M <= MAX_M && k >= 1 && k <= MAX_K && nprobe >= 1 && nprobe <= MAX_NLIST,
               "at_ivfpq_search_limits: bad sizes M=%d nprobe=%d k=%d", M, nprobe, k);
    if (pairs_per_block) *pairs_per_block = queries_per_block(M);
    if (rows_per_group) *rows_per_group = GROUP;
    if (queries_per_chunk_out) *queries_per_chunk_out = queries_per_chunk(nprobe, k);
    return AT_OK;
}

extern "C" int at_ivfpq_build(at_ctx* ctx, const uint8_t* codes, const int64_t* lists, const int64_t* order, int64_t ntotal,
                              int M, int nlist, int ngroups, uint8_t* grouped, int32_t* pos2id, int32_t* first,
                              void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_ivfpq_build: ctx is null");
    AT_REQUIRE(ntotal >= 0 && ntotal < ((int64_t)1 << 31) && M >= 1 && M <= MAX_M && nlist >= 1 && nlist <= MAX_NLIST,
               "at_ivfpq_build: bad sizes ntotal=%lld (below 2^31) M=%d (1 .. %d) nlist=%d", (long long)ntotal, M, MAX_M,
               nlist);
    AT_REQUIRE(ngroups >= ntotal / GROUP + nlist && (int64_t)ngroups * GROUP < ((int64_t)1 << 31),
               "at_ivfpq_build: ngroups=%d (at least ntotal / %d + nlist = %lld, and below 2^31 positions)", ngroups, GROUP,
               (long long)(ntotal / GROUP + nlist));
    AT_REQUIRE(grouped && pos2id && first && ((codes && lists && order) || ntotal == 0), "at_ivfpq_build: null pointer");
    AT_HIP(hipSetDevice(ctx->device));
    int rc = at_guard_enter(&ctx->guard[AT_GUARD_IVFPQ], stream);
    if (rc) return rc;
    const size_t b_cnt = ws_align(sizeof(int) * (size_t)nlist), b_tab = ws_align(sizeof(int) * ((size_t)nlist + 1));
    unsigned char* w = static_cast<unsigned char*>(at_ws(ctx, WS_IVFPQ, b_cnt + b_tab, stream));
    if (!w) return AT_E_NOMEM;
    int* cnt = reinterpret_cast<int*>(w);
    int* start = reinterpret_cast<int*>(w + b_cnt);
    AT_HIP(hipMemsetAsync(cnt, 0, b_cnt, stream));
    if (ntotal > 0)
        AT_LAUNCH(ivf_count_kernel, dim3((unsigned)((ntotal + WG - 1) / WG)), dim3(WG), 0, stream,
                  reinterpret_cast<const long*>(lists), (long)ntotal, nlist, cnt);
    AT_LAUNCH(ivf_offsets_kernel, dim3(1), dim3(WG), 0, stream, cnt, nlist, GROUP, start, first);
    AT_LAUNCH(ivfpq_group_kernel, dim3((unsigned)(((int64_t)ngroups * GROUP + WG - 1) / WG)), dim3(WG), 0, stream, codes,
              reinterpret_cast<const long*>(lists), reinterpret_cast<const long*>(order), (long)ntotal, M, nlist, start,
              first, ngroups, grouped, pos2id);
    return at_guard_leave(&ctx->guard[AT_GUARD_IVFPQ], stream);
}

extern "C" int at_ivfpq_search_f32(at_ctx* ctx, const float* x, int64_t n, int d, const int64_t* probes, int nprobe,
                                   int nlist, const float* centroids_or_null, int M, int ksub, const float* codebooks,
                                   const uint8_t* grouped, int ngroups, const int32_t* pos2id, const int32_t* first,
                                   int64_t ntotal, int k, int64_t* ids, float* dist, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_ivfpq_search_f32: ctx is null");
    AT_REQUIRE(k >= 1 && k <= MAX_K, "at_ivfpq_search_f32: k = %d (1 .. %d)", k, MAX_K);
    AT_REQUIRE(nprobe >= 1 && nprobe <= MAX_NLIST, "at_ivfpq_search_f32: nprobe = %d (at least 1)", nprobe);
    AT_REQUIRE(n >= 0 && d >= 1 && M >= 1 && M <= MAX_M && d % M == 0 && ksub >= 1 && ksub <= 256 && nlist >= 1 &&
                   nlist <= MAX_NLIST && ntotal >= 0 && ntotal < ((int64_t)1 << 31) && ngroups >= 1 &&
                   (int64_t)ngroups * GROUP < ((int64_t)1 << 31),
               "at_ivfpq_search_f32: bad sizes n=%lld d=%d M=%d (1 .. %d, dividing d) ksub=%d nlist=%d ntotal=%lld (below "
               "2^31) ngroups=%d", (long long)n, d, M, MAX_M, ksub, nlist, (long long)ntotal, ngroups);
    if (n == 0) return AT_OK;
    AT_REQUIRE(x && probes && codebooks && grouped && pos2id && first && ids, "at_ivfpq_search_f32: null pointer");
    AT_REQUIRE(n <= ((int64_t)1 << 38) / (d > k ? d : k), "at_ivfpq_search_f32: n=%lld too large", (long long)n);
    AT_HIP(hipSetDevice(ctx->device));

    // queries in chunks whose partial lists stay within the budget
    const size_t per_query = sizeof(uint64_t) * (size_t)nprobe * k;
    int64_t chunk = queries_per_chunk(nprobe, k);
    if (chunk > n) chunk = n;
    const int qb = queries_per_block(M);
    int rc = at_guard_enter(&ctx->guard[AT_GUARD_IVFPQ], stream);
    if (rc) return rc;
    const size_t b_part = ws_align(per_query * (size_t)chunk), b_pair = ws_align(sizeof(int) * (size_t)chunk * nprobe);
    const size_t b_cnt = ws_align(sizeof(int) * 2 * (size_t)nlist), b_tab = ws_align(sizeof(int) * ((size_t)nlist + 1));
    unsigned char* w = static_cast<unsigned char*>(at_ws(ctx, WS_IVFPQ, b_part + b_pair + b_cnt + 2 * b_tab, stream));
    if (!w) return AT_E_NOMEM;
    ScanArgs a;
    a.d = d; a.M = M; a.ksub = ksub; a.cb = codebooks; a.cent = centroids_or_null; a.nprobe = nprobe; a.nlist = nlist;
    a.codes = grouped; a.first = first; a.ngroups = ngroups; a.pos2id = pos2id; a.ntotal = ntotal; a.k = k;
    a.partial = reinterpret_cast<uint64_t*>(w);
    int* pairtab = reinterpret_cast<int*>(w + b_part);
    int* cnt = reinterpret_cast<int*>(w + b_part + b_pair);   // [nlist] counts, then [nlist] cursors
    int* pair_start = reinterpret_cast<int*>(w + b_part + b_pair + b_cnt);
    int* blk_start = reinterpret_cast<int*>(w + b_part + b_pair + b_cnt + b_tab);
    a.pairtab = pairtab; a.pair_start = pair_start; a.blk_start = blk_start;

    for (int64_t q0 = 0; q0 < n; q0 += chunk) {
        const int64_t nq = n - q0 < chunk ? n - q0 : chunk;
        a.ptotal = (int)(nq * nprobe);
        a.x = x + q0 * d;
        const long* pq = reinterpret_cast<const long*>(probes + q0 * nprobe);
        const unsigned pgrid = (unsigned)((a.ptotal + WG - 1) / WG);
        AT_HIP(hipMemsetAsync(cnt, 0, b_cnt, stream));
        AT_LAUNCH(ivf_count_kernel, dim3(pgrid), dim3(WG), 0, stream, pq, (long)a.ptotal, nlist, cnt);
        AT_LAUNCH(ivf_offsets_kernel, dim3(1), dim3(WG), 0, stream, cnt, nlist, qb, pair_start, blk_start);
        AT_LAUNCH(ivf_scatter_kernel, dim3(pgrid), dim3(WG), 0, stream, pq, a.ptotal, nlist, pair_start, cnt + nlist,
                  pairtab, a.partial, k);
        rc = qb == 4 ? launch_scan_by_width<4>(ctx, a, stream) : launch_scan_by_width<2>(ctx, a, stream);
        if (rc) return rc;
        AT_LAUNCH(pq_merge_kernel, dim3((unsigned)nq), dim3(WG), 0, stream, a.partial, (long)nprobe * k, k,
                  reinterpret_cast<long*>(ids + q0 * k), dist ? dist + q0 * k : nullptr);
    }
    return at_guard_leave(&ctx->guard[AT_GUARD_IVFPQ], stream);
}
