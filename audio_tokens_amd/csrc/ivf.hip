// ivf.hip -- inverted lists over exact fp32 rows on gfx950: at_ivf_build_f32, at_ivf_search_f32 (ops.IndexIVFFlat).
// Contract: include/audio_tokens_amd.h, DESIGN.md section 6o.
//
// Arithmetic: dis(i, r) between query i and stored row r is ALWAYS the expansion form of at_assign_f32 -- ip, |x|^2,
// |r|^2 ascending fmaf chains (v_mfma_f32_32x32x2_f32 for ip), dis = (xn + rn) - 2*ip in one fma, the clamp
// v < 0 ? 0 : v that leaves a NaN a NaN -- whatever n is: a query meets its stored rows in blocks made of whoever else
// probes the same list, so "the call has n < 20 rows" says nothing about the shape any distance is computed in.
//
// The image (at_ivf_build_f32): chunked_sweep.h's chunked image with the stored rows in the centroids' role, grouped
// by list in ascending id (the caller's stable order), every list padded to whole tiles of TILE = 128 rows.  A pad row
// is all +0 with norm +inf, so it is never listed.  first[l] is the first tile of list l, first[nlist] the number of
// tiles in use; pos2id[position] is the id of the row at a position of the image, -1 for a pad.
//
// The search (at_ivf_search_f32), per chunk of queries, all on the stream:
//   count / offsets / scatter: a counting sort of the (query, probe) pairs with a list in [0, nlist) by list -- pair p =
//     query * nprobe + probe slot lands somewhere in pairtab[pair_start[l] .. pair_start[l + 1]); where exactly is
//     decided by an atomic and does not matter, a query's result does not depend on the lane that computes it --, and
//     blk_start[l], the prefix sum of the numbers of 128-pair blocks per list;
//   scan: workgroup b takes the (list, block of up to 128 probing queries) it finds by a binary search of b in
//     blk_start, gathers its queries through pairtab as the MFMA B operand (32 per wave), streams the tiles
//     [first[l], first[l + 1]) through cs::Sweep and keeps topk_lanes.h's per-lane list of (dis, position).  Positions
//     ascend with the id inside a list, so the strict `<` insert keeps the lexicographic (dis, id) order.  It writes k
//     keys (distance bits << 32) | id per pair, -0 as +0, KEY_NONE in the places left over; distances are >= +0, so
//     the keys order as unsigned integers;
//   merge: one wave per query picks the k smallest of its nprobe * k keys, one per round (the smallest key above the
//     one before), and writes ids and distances, (-1, +inf) behind the last.
//
// Every index that addresses memory is derived from tables this file builds, and is checked against the host-side
// bound of the array it addresses before it is used (the comments at each use say which construction makes the check
// a formality).
#include "at_internal.h"
#include "chunked_sweep.h"
#include "pair_inversion.h"
#include "topk_lanes.h"

namespace {

constexpr int WG = 256;              // 4 waves
constexpr int NA = 4;                // 32-row accumulators per tile
constexpr int TILE = cs::tile_rows(NA);   // 128 stored rows
constexpr int QB = 128;              // probing queries per workgroup of the scan: 32 per wave
constexpr int MAX_K = 32;            // the per-lane list: knn.hip's K_FUSED
constexpr int MAX_NLIST = 1 << 24;
constexpr size_t BUDGET_BYTES = (size_t)256 << 20;   // the partial lists of one chunk of queries
constexpr int64_t MAX_PAIRS = (int64_t)1 << 30;      // (query, probe) pairs of one chunk: pair indices are ints
constexpr uint64_t KEY_NONE = ~(uint64_t)0;

// the counting sort of the pairs and list_of_unit: pair_inversion.h (shared with ivfpq.hip)
using pinv::ivf_count_kernel;
using pinv::ivf_offsets_kernel;
using pinv::ivf_scatter_kernel;
using pinv::list_of_unit;

// one workgroup per tile of the image
__global__ void __launch_bounds__(WG)
ivf_image_kernel(const float* __restrict__ rows, const long* __restrict__ lists, const long* __restrict__ order,
                 long ntotal, int d, int nchunks, int nlist, const int* __restrict__ start,
                 const int* __restrict__ first, float* __restrict__ img, int* __restrict__ pos2id) {
    __shared__ long src[TILE];
    const int t = blockIdx.x;
    // a tile behind the last list (the host's bound is not tight) is all pads and never read
    int l = -1, base = 0, cnt = 0, s0 = 0;
    if (t < first[nlist]) {
        l = list_of_unit(first, nlist, t);
        base = (t - first[l]) * TILE;
        s0 = start[l];
        cnt = start[l + 1] - s0;
    }
    for (int r = threadIdx.x; r < TILE; r += WG) {
        long id = -1;
        const long p = (long)s0 + base + r;
        // p < start[l + 1] <= ntotal by the prefix sum; the row it names must be one of list l, or `order` is not what
        // the contract asks for and the position stays a pad
        if (base + r < cnt && p >= 0 && p < ntotal) {
            id = order[p];
            if (id < 0 || id >= ntotal || lists[id] != l) id = -1;
        }
        src[r] = id;
        pos2id[(size_t)t * TILE + r] = (int)id;
    }
    __syncthreads();
    float* out = img + (size_t)t * cs::tile_floats(NA, nchunks);
    constexpr int slots = cs::DC / 4;   // 16-byte slots per row piece
    for (int e = threadIdx.x; e < nchunks * TILE * slots; e += WG) {
        const int ch = e / (TILE * slots);
        const int r = (e / slots) % TILE, pc = e % slots;
        const long id = src[r];
        *reinterpret_cast<f32x4*>(out + ((size_t)ch * TILE + r) * cs::DC + pc * 4) =
            cs::image_slot(id >= 0 ? rows + (size_t)id * d : nullptr, d, ch * cs::DC, r, pc);
    }
    for (int r = threadIdx.x; r < cs::CN_PAD; r += WG) {
        const long id = r < TILE ? src[r] : -1;
        out[(size_t)cs::piece_floats(NA) * nchunks + r] = cs::image_norm(id >= 0 ? rows + (size_t)id * d : nullptr, d);
    }
}

// NCH > 0: d = 64 * NCH, the query chunks in registers; NCH = 0: any d % 4 == 0, the chunk re-read per stage
template <int NCH, int KL>
__global__ void __launch_bounds__(WG, 2)
ivf_scan_kernel(const float* __restrict__ X, int d, int nchunks, int nprobe, int ptotal, int nlist,
                const int* __restrict__ pair_start, const int* __restrict__ blk_start,
                const int* __restrict__ pairtab, const float* __restrict__ img, const int* __restrict__ first,
                int ntiles_cap, const int* __restrict__ pos2id, long ntotal, int k, uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 2 * cs::buf_floats(NA) floats
    // The grid is the host's bound; the workgroups behind the real count leave as a whole, before the first barrier.
    // Everything up to the sweep is the same in every thread of the workgroup.
    const int b = blockIdx.x;
    if (b >= blk_start[nlist]) return;
    const int l = list_of_unit(blk_start, nlist, b);
    // blk_start[l] <= b < blk_start[l + 1] = blk_start[l] + ceil(c / QB), c the pairs of list l:
    // (b - blk_start[l]) * QB < c, so the block holds 1 .. QB pairs, all inside the list's stretch of pairtab
    const int p0 = pair_start[l] + (b - blk_start[l]) * QB;
    int cnt = pair_start[l + 1] - p0;
    if (cnt > QB) cnt = QB;
    if (cnt < 1 || p0 < 0 || p0 + cnt > ptotal) return;
    // first ascends and first[nlist] <= ntiles_cap (the host's bound on the tiles of the image)
    int t0 = first[l], t1 = first[l + 1];
    if (t0 < 0) t0 = 0;
    if (t1 > ntiles_cap) t1 = ntiles_cap;
    const int ntiles = t1 - t0;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int slot = wave * 32 + j;
    bool valid = slot < cnt;
    // a lane behind the block's count computes the block's first pair again and stores nothing (knn.hip's r = n - 1)
    int pair = pairtab[p0 + (valid ? slot : 0)];
    if (pair < 0 || pair >= ptotal) {   // pairtab holds pair indices < ptotal only (ivf_scatter_kernel)
        pair = 0;
        valid = false;
    }
    uint64_t* out = partial + (size_t)pair * k;
    if (ntiles <= 0) {   // an empty list: nothing to stream (and no tile of its own to prime the stream with)
        if (valid && h == 0)
            for (int s = 0; s < k; s++) out[s] = KEY_NONE;
        return;
    }
    const bool live = wave * 32 < cnt;   // a wave without a query still feeds the stream and meets the barriers

    const int nch = NCH > 0 ? NCH : nchunks;
    cs::Sweep<NA, NCH, true> sweep(img + (size_t)t0 * cs::tile_floats(NA, nch), smem, nchunks, ntiles);
    const int dd = NCH > 0 ? NCH * cs::DC : d;
    const float* xrow = X + (size_t)(pair / nprobe) * dd;   // pair / nprobe < ptotal / nprobe = the chunk's queries
    const float xn = cs::sqnorm16(xrow, dd);
    float xr[NCH > 0 ? NCH : 1][cs::DC / 2];
    if constexpr (NCH > 0) {
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) cs::load_x_chunk(xrow, ch, dd, h, xr[ch]);
    }

    float ld[KL];
    unsigned li[KL];
    tk::clear<KL>(ld, li);

    // (the stage is written out here as in knn.hip, see there)
    f32x16 acc[NA];
    auto stage = [&](int s, int ct, int ch, const float (&xv)[cs::DC / 2]) {
        const float* cur = sweep.begin_stage(smem, s, ct, ch);
        if (live) {
            sweep.mfma_piece(acc, cur, xv, ch == 0);
            if (ch == sweep.nch - 1) {
                const float* cnorm = cur + sweep.PIECE_F;   // the tile's norms
#pragma unroll
                for (int a = 0; a < NA; a++) {
                    float u[16];
                    tk::l2_of_acc16(acc[a], cnorm + a * 32 + 4 * h, xn, u);
                    tk::offer16<KL>(ld, li, u, (unsigned)cs::acc_base(ct * NA + a, h));
                }
            }
        }
        __syncthreads();
    };
    sweep.prime();
    if constexpr (NCH > 0) {
        for (int ct = 0; ct < ntiles; ct++) {
            stage(ct * NCH, ct, 0, xr[0]);
            if constexpr (NCH == 2) stage(ct * NCH + 1, ct, 1, xr[NCH - 1]);
        }
    } else {
        int ct = 0, ch = 0;
        for (int s = 0; s < sweep.nstages; s++) {
            if (live) cs::load_x_chunk(xrow, ch, d, h, xr[0]);
            stage(s, ct, ch, xr[0]);
            if (++ch == sweep.nch) { ch = 0; ct++; }
        }
    }

    float cd[KL];
    unsigned ci[KL];
    tk::merge_halves<KL>(ld, li, cd, ci);
    if (h == 0 && valid) {
#pragma unroll
        for (int s = 0; s < KL; s++) {
            if (s < k) {
                uint64_t key = KEY_NONE;
                // a listed position is one of the tiles [t0, t1): below ntiles_cap * TILE, the length of pos2id
                if (ci[s] < (unsigned)ntiles * TILE) {
                    const long id = pos2id[(size_t)t0 * TILE + ci[s]];
                    const unsigned bits = cd[s] == 0.0f ? 0u : __float_as_uint(cd[s]);   // -0 -> +0
                    if (id >= 0 && id < ntotal) key = ((uint64_t)bits << 32) | (uint64_t)id;
                }
                out[s] = key;
            }
        }
    }
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// one wave per query: the k smallest of its `total` keys (KEY_NONE: an empty place), ascending
__global__ void __launch_bounds__(WG)
ivf_merge_kernel(const uint64_t* __restrict__ partial, int nq, int total, int k, long* __restrict__ ids,
                 float* __restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;   // (no barrier in this kernel)
    const uint64_t* src = partial + (size_t)q * total;
    uint64_t prev = 0;
    for (int s = 0; s < k; s++) {
        uint64_t best = KEY_NONE;
        if (s == 0 || prev != KEY_NONE) {
            for (int t = lane; t < total; t += 64) {
                const uint64_t key = src[t];
                if ((s == 0 || key > prev) && key < best) best = key;
            }
            best = wave_min_u64(best);
        }
        if (lane == 0) {
            const bool has = best != KEY_NONE;
            ids[(size_t)q * k + s] = has ? (long)(uint32_t)best : -1L;
            if (dist) dist[(size_t)q * k + s] = has ? __uint_as_float((uint32_t)(best >> 32)) : __builtin_inff();
        }
        prev = best;
    }
}

template <int NCH, int KL>
int launch_scan(at_ctx* ctx, unsigned grid, const float* x, int d, int nprobe, int ptotal, int nlist, const int* pair_start,
                const int* blk_start, const int* pairtab, const float* img, const int* first, int ntiles,
                const int* pos2id, int64_t ntotal, int k, uint64_t* partial, hipStream_t stream) {
    const size_t lds = 2 * sizeof(float) * cs::buf_floats(NA);
    AT_RAISE_LDS(ctx, (ivf_scan_kernel<NCH, KL>), lds);
    AT_LAUNCH((ivf_scan_kernel<NCH, KL>), dim3(grid), dim3(WG), lds, stream, x, d, cs::nchunks_of(d), nprobe, ptotal, nlist,
              pair_start, blk_start, pairtab, img, first, ntiles, pos2id, (long)ntotal, k, partial);
    return AT_OK;
}

template <int KL, typename... A>
int launch_scan_by_d(at_ctx* ctx, unsigned grid, const float* x, int d, A... a) {
    if (d == 64) return launch_scan<1, KL>(ctx, grid, x, d, a...);
    if (d == 128) return launch_scan<2, KL>(ctx, grid, x, d, a...);
    return launch_scan<0, KL>(ctx, grid, x, d, a...);
}

size_t ivf_align(size_t b) { return (b + 255) & ~size_t(255); }

}  // namespace

extern "C" int at_ivf_build_f32(at_ctx* ctx, const float* rows, const int64_t* lists, const int64_t* order, int64_t ntotal,
                                int d, int nlist, int ntiles, float* img, int32_t* pos2id, int32_t* first, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_ivf_build_f32: ctx is null");
    AT_REQUIRE(ntotal >= 0 && ntotal < ((int64_t)1 << 31) && d >= 1 && nlist >= 1 && nlist <= MAX_NLIST,
               "at_ivf_build_f32: bad sizes ntotal=%lld (below 2^31) d=%d nlist=%d", (long long)ntotal, d, nlist);
    AT_REQUIRE(ntiles >= ntotal / TILE + nlist && (int64_t)ntiles * TILE < ((int64_t)1 << 31),
               "at_ivf_build_f32: ntiles=%d (at least ntotal / %d + nlist = %lld, and below 2^31 positions)", ntiles, TILE,
               (long long)(ntotal / TILE + nlist));
    AT_REQUIRE(img && pos2id && first && ((rows && lists && order) || ntotal == 0), "at_ivf_build_f32: null pointer");
    AT_HIP(hipSetDevice(ctx->device));
    int rc = at_guard_enter(&ctx->guard[AT_GUARD_IVF], stream);
    if (rc) return rc;
    const size_t b_cnt = ivf_align(sizeof(int) * (size_t)nlist), b_tab = ivf_align(sizeof(int) * ((size_t)nlist + 1));
    unsigned char* w = static_cast<unsigned char*>(at_ws(ctx, WS_IVF, b_cnt + b_tab, stream));
    if (!w) return AT_E_NOMEM;
    int* cnt = reinterpret_cast<int*>(w);
    int* start = reinterpret_cast<int*>(w + b_cnt);
    AT_HIP(hipMemsetAsync(cnt, 0, b_cnt, stream));
    if (ntotal > 0)
        AT_LAUNCH(ivf_count_kernel, dim3((unsigned)((ntotal + WG - 1) / WG)), dim3(WG), 0, stream,
                  reinterpret_cast<const long*>(lists), (long)ntotal, nlist, cnt);
    AT_LAUNCH(ivf_offsets_kernel, dim3(1), dim3(WG), 0, stream, cnt, nlist, TILE, start, first);
    AT_LAUNCH(ivf_image_kernel, dim3((unsigned)ntiles), dim3(WG), 0, stream, rows, reinterpret_cast<const long*>(lists),
              reinterpret_cast<const long*>(order), (long)ntotal, d, cs::nchunks_of(d), nlist, start, first, img, pos2id);
    return at_guard_leave(&ctx->guard[AT_GUARD_IVF], stream);
}

extern "C" int at_ivf_search_f32(at_ctx* ctx, const float* x, int64_t n, int d, const int64_t* probes, int nprobe,
                                 int nlist, const float* img, int ntiles, const int32_t* pos2id, const int32_t* first,
                                 int64_t ntotal, int k, int64_t* ids, float* dist, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_ivf_search_f32: ctx is null");
    AT_REQUIRE(k >= 1 && k <= MAX_K, "at_ivf_search_f32: k = %d (1 .. %d)", k, MAX_K);
    AT_REQUIRE(nprobe >= 1 && nprobe <= MAX_NLIST, "at_ivf_search_f32: nprobe = %d (at least 1)", nprobe);
    AT_REQUIRE(n >= 0 && d >= 1 && d % 4 == 0 && nlist >= 1 && nlist <= MAX_NLIST && ntotal >= 0 &&
                   ntotal < ((int64_t)1 << 31) && ntiles >= 1 && (int64_t)ntiles * TILE < ((int64_t)1 << 31),
               "at_ivf_search_f32: bad sizes n=%lld d=%d (a multiple of 4) nlist=%d ntotal=%lld (below 2^31) ntiles=%d",
               (long long)n, d, nlist, (long long)ntotal, ntiles);
    if (n == 0) return AT_OK;
    AT_REQUIRE(x && probes && img && pos2id && first && ids, "at_ivf_search_f32: null pointer");
    AT_REQUIRE(at_aligned16(x) && at_aligned16(img), "at_ivf_search_f32: x and the image must be 16-byte aligned");
    AT_REQUIRE(n <= ((int64_t)1 << 38) / (d > k ? d : k), "at_ivf_search_f32: n=%lld too large", (long long)n);
    AT_HIP(hipSetDevice(ctx->device));

    // queries in chunks whose partial lists stay within the budget
    const size_t per_query = sizeof(uint64_t) * (size_t)nprobe * k;
    int64_t chunk = (int64_t)(BUDGET_BYTES / per_query);
    if (chunk > MAX_PAIRS / nprobe) chunk = MAX_PAIRS / nprobe;
    if (chunk < 1) chunk = 1;
    if (chunk > n) chunk = n;
    int rc = at_guard_enter(&ctx->guard[AT_GUARD_IVF], stream);
    if (rc) return rc;
    const size_t b_part = ivf_align(per_query * (size_t)chunk), b_pair = ivf_align(sizeof(int) * (size_t)chunk * nprobe);
    const size_t b_cnt = ivf_align(sizeof(int) * 2 * (size_t)nlist), b_tab = ivf_align(sizeof(int) * ((size_t)nlist + 1));
    unsigned char* w = static_cast<unsigned char*>(at_ws(ctx, WS_IVF, b_part + b_pair + b_cnt + 2 * b_tab, stream));
    if (!w) return AT_E_NOMEM;
    uint64_t* partial = reinterpret_cast<uint64_t*>(w);
    int* pairtab = reinterpret_cast<int*>(w + b_part);
    int* cnt = reinterpret_cast<int*>(w + b_part + b_pair);   // [nlist] counts, then [nlist] cursors
    int* pair_start = reinterpret_cast<int*>(w + b_part + b_pair + b_cnt);
    int* blk_start = reinterpret_cast<int*>(w + b_part + b_pair + b_cnt + b_tab);

    for (int64_t q0 = 0; q0 < n; q0 += chunk) {
        const int64_t nq = n - q0 < chunk ? n - q0 : chunk;
        const int ptotal = (int)(nq * nprobe);
        const float* xq = x + q0 * d;
        const long* pq = reinterpret_cast<const long*>(probes + q0 * nprobe);
        const unsigned pgrid = (unsigned)((ptotal + WG - 1) / WG);
        AT_HIP(hipMemsetAsync(cnt, 0, b_cnt, stream));
        AT_LAUNCH(ivf_count_kernel, dim3(pgrid), dim3(WG), 0, stream, pq, (long)ptotal, nlist, cnt);
        AT_LAUNCH(ivf_offsets_kernel, dim3(1), dim3(WG), 0, stream, cnt, nlist, QB, pair_start, blk_start);
        AT_LAUNCH(ivf_scatter_kernel, dim3(pgrid), dim3(WG), 0, stream, pq, ptotal, nlist, pair_start, cnt + nlist, pairtab,
                  partial, k);
        // sum over the lists of ceil(c / QB) <= ptotal / QB + the number of probed lists
        const unsigned grid = (unsigned)(ptotal / QB + (nlist < ptotal ? nlist : ptotal));
        if (k <= 4) rc = launch_scan_by_d<4>(ctx, grid, xq, d, nprobe, ptotal, nlist, pair_start, blk_start, pairtab, img, first, ntiles, pos2id, ntotal, k, partial, stream);
        else if (k <= 8) rc = launch_scan_by_d<8>(ctx, grid, xq, d, nprobe, ptotal, nlist, pair_start, blk_start, pairtab, img, first, ntiles, pos2id, ntotal, k, partial, stream);
        else if (k <= 16) rc = launch_scan_by_d<16>(ctx, grid, xq, d, nprobe, ptotal, nlist, pair_start, blk_start, pairtab, img, first, ntiles, pos2id, ntotal, k, partial, stream);
        else rc = launch_scan_by_d<32>(ctx, grid, xq, d, nprobe, ptotal, nlist, pair_start, blk_start, pairtab, img, first, ntiles, pos2id, ntotal, k, partial, stream);
        if (rc) return rc;
        AT_LAUNCH(ivf_merge_kernel, dim3((unsigned)((nq + WG / 64 - 1) / (WG / 64))), dim3(WG), 0, stream, partial, (int)nq,
                  nprobe * k, k, reinterpret_cast<long*>(ids + q0 * k), dist ? dist + q0 * k : nullptr);
    }
    return at_guard_leave(&ctx->guard[AT_GUARD_IVF], stream);
}
