// pq_search.hip -- asymmetric-distance search over product-quantiser codes on gfx950: at_pq_search_f32
// (ops.IndexPQ.search).  Contract: include/audio_tokens_amd.h, DESIGN.md section 6n.
//
// A query row x[i] gets the table T[i][m][j] = sum_f (x[i][m * dsub + f] - cb[m][j][f])^2 -- always the direct form:
// df = x - c, acc = fmaf(df, df, acc) from +0 over f ascending -- and database row r the distance
// T[i][0][codes[r][0]] + T[i][1][codes[r][1]] + ..., one fp32 addition per step in ascending m.  Every term is >= +0, so a
// distance below +inf has the sign bit clear and its bit pattern orders as an unsigned integer:
// key = (bits << 32) | r orders (distance, id) lexicographically.  Row i of the result holds the k smallest keys.
//
// Scan kernel: grid (blocks of QB queries) x (slabs of SLAB database rows); QB = 4 for M <= 32, 2 above (the tables of a
// block: M * ksub * QB floats, at most 128 KiB of LDS).  A workgroup
//   * builds the tables of its queries, one thread per (m, j) entry and all QB queries in that thread, so the codebook
//     word is read once; the entry is stored with the queries innermost, lut[m][j][q]: one ds_read_b128 (QB = 4) or
//     ds_read_b64 (QB = 2) at (m, code) returns the entries of all the block's queries;
//   * streams the code rows of its slab once, a row per thread and round of WG rows: 16-, 8- or 4-byte loads where M and
//     the pointer allow, byte loads otherwise, the next piece requested before the current one is looked up;
//   * keeps, per query, a buffer of candidate keys in LDS and a threshold key in registers: a candidate is appended (LDS
//     atomic on a counter for its slot) only if its key is below the threshold; when a buffer could overflow in the next
//     round it is sorted (bitonic, the whole workgroup), cut to the k smallest keys, and the k-th becomes the threshold.
//     The threshold starts at the key of (+inf, 0): a NaN or +inf distance never passes.  What is kept is decided by the key
//     alone -- the slot an atomic hands out only says where a key waits for the next sort --, and an equal distance with
//     a lower id is a smaller key, so it passes;
//   * ends with a sort and writes its k smallest keys (padded with KEY_NONE) to the workspace.
// The round's counter rotates over three words: the word of round r is read by every thread behind the barrier of round
// r, cleared in round r + 2 by a thread that has passed the barrier of round r + 1 (which every thread reaches only
// after its read), and used again in round r + 3: one barrier per round.  The three words sit in the last two places of
// the query's buffer, which the keys never reach, so the LDS of a workgroup is the tables and QB * CAP keys exactly:
// at M = 16 that is 80 KiB, and two workgroups share a CU.
// A stored code >= ksub (possible only with ksub < 256) is clamped for the look-up and makes the row unlisted.
//
// Merge kernel: one workgroup per query streams the nslabs * k keys of the query's lists through the same buffer and
// writes ids and distances, (-1, +inf) behind the last listed row.  (It lives in pq_keys.h with the buffer's sorts and
// the code-row pieces: ivfpq.hip shares them.)
//
// Host: queries in chunks whose lists (8 bytes per (query, slab, place)) stay within BUDGET_BYTES; two launches per
// chunk; nothing is read back and nothing waits on the host.
#include "at_internal.h"
#include "pq_keys.h"

namespace {

// the candidate buffer, its sorts, the merge and the code-row pieces: pq_keys.h (shared with ivfpq.hip)
using namespace pqk;
constexpr int SLAB = 65536;          // database rows per workgroup: M * SLAB look-ups against 256 * d fmaf per query
constexpr size_t BUDGET_BYTES = (size_t)256 << 20;   // the lists of one chunk of queries
constexpr int64_t MAX_CHUNK = ((int64_t)1 << 24) - 4;   // the merge is a workgroup per query: chunk * WG work-items < 2^32

struct Plan {
    int qb;
    int64_t nslabs, chunk;   // chunk: queries per pair of launches, a multiple of qb
    size_t per_query;        // bytes of lists
};

Plan make_plan(int M, int64_t ntotal, int k) {
    Plan p;
    p.qb = queries_per_block(M);
    p.nslabs = (ntotal + SLAB - 1) / SLAB;
    if (p.nslabs < 1) p.nslabs = 1;
    p.per_query = sizeof(uint64_t) * (size_t)p.nslabs * k;   // <= 32 MiB (ntotal < 2^31, k <= 128)
    p.chunk = (int64_t)(BUDGET_BYTES / p.per_query);
    if (p.chunk > MAX_CHUNK) p.chunk = MAX_CHUNK;
    p.chunk -= p.chunk % p.qb;
    return p;
}

// QB queries per workgroup, code rows in pieces of W bytes (M % W == 0, codes W-byte aligned), FULL: ksub == 256
template <int QB, int W, bool FULL>
__global__ void __launch_bounds__(WG)
pq_scan_kernel(const float* __restrict__ x, long n, int d, int M, int ksub, const float* __restrict__ cb,
               const uint8_t* __restrict__ codes, long ntotal, int k, uint64_t* __restrict__ lists) {
    typedef float fq __attribute__((ext_vector_type(QB)));
    typedef typename Piece<W>::type piece_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int entries = M * ksub;
    fq* lut = reinterpret_cast<fq*>(smem);                                           // [M][ksub][QB]
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem + sizeof(float) * QB * (size_t)entries);   // [QB][CAP]
    auto counters = [&](int q) { return reinterpret_cast<int*>(buf + q * CAP + CAP - 2); };   // three words per query
    const int tid = threadIdx.x;
    const long q0 = (long)blockIdx.x * QB;
    const int dsub = d / M;

    for (int e = tid; e < entries; e += WG) {
        const int m = e / ksub;
        const float* c = cb + (size_t)e * dsub;
        const float* xq[QB];
        float acc[QB];
#pragma unroll
        for (int q = 0; q < QB; q++) {
            const long qi = q0 + q < n ? q0 + q : n - 1;   // (a slot behind the last query recomputes it and stores nothing)
            xq[q] = x + qi * (long)d + m * dsub;
            acc[q] = 0.0f;
        }
        for (int f = 0; f < dsub; f++) {
            const float cf = c[f];
#pragma unroll
            for (int q = 0; q < QB; q++) {
                const float df = xq[q][f] - cf;
                acc[q] = __builtin_fmaf(df, df, acc[q]);
            }
        }
        fq v;
#pragma unroll
        for (int q = 0; q < QB; q++) v[q] = acc[q];
        lut[e] = v;
    }
    if (tid < 3 * QB) counters(tid / 3)[tid % 3] = 0;
    __syncthreads();

    const long s0 = (long)blockIdx.y * SLAB;
    const long s1 = s0 + SLAB < ntotal ? s0 + SLAB : ntotal;
    const int npieces = M / W;
    int base[QB];
    uint64_t thr[QB];   // the same in every thread
#pragma unroll
    for (int q = 0; q < QB; q++) {
        base[q] = 0;
        thr[q] = KEY_LIMIT;
    }
    int cur = 0;

    piece_t v = piece_t();
    if (s0 + tid < s1) v = *reinterpret_cast<const piece_t*>(codes + (s0 + tid) * (long)M);
    for (long r0 = s0; r0 < s1; r0 += WG) {
        const long row = r0 + tid;
        const bool valid = row < s1;
        bool listed = valid;
        fq acc;
#pragma unroll
        for (int q = 0; q < QB; q++) acc[q] = 0.0f;
        for (int p = 0; p < npieces; p++) {
            piece_t nx = piece_t();
            if (p + 1 < npieces) {
                if (valid) nx = *reinterpret_cast<const piece_t*>(codes + row * (long)M + (p + 1) * W);
            } else if (row + WG < s1) {
                nx = *reinterpret_cast<const piece_t*>(codes + (row + WG) * (long)M);
            }
#pragma unroll
            for (int b = 0; b < W; b++) {
                unsigned code = piece_byte<W>(v, b);
                const int m = p * W + b;
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
                const uint64_t key = ((uint64_t)__float_as_uint(acc[q]) << 32) | (uint32_t)row;
                if (key < thr[q]) {
                    const int s = base[q] + atomicAdd(counters(q) + cur, 1);
                    buf[q * CAP + s] = key;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < QB; q++) {
            base[q] += counters(q)[cur];
            if (base[q] > FULL_AT) base[q] = cut_to_k(buf + q * CAP, thr[q], base[q], k);
        }
        cur = nxt;
    }

#pragma unroll
    for (int q = 0; q < QB; q++) {
        sort_keys(buf + q * CAP, base[q]);
        const int cnt = base[q] < k ? base[q] : k;
        if (q0 + q < n) {
            uint64_t* out = lists + ((q0 + q) * (long)gridDim.y + blockIdx.y) * k;
            for (int t = tid; t < k; t += WG) out[t] = t < cnt ? buf[q * CAP + t] : KEY_NONE;
        }
    }
}

size_t scan_lds_bytes(int qb, int M, int ksub) {
    return sizeof(float) * qb * (size_t)M * ksub + sizeof(uint64_t) * qb * CAP;
}

template <int QB, int W>
int launch_scan(at_ctx* ctx, const float* x, int64_t n, int d, int M, int ksub, const float* cb, const uint8_t* codes,
                int64_t ntotal, int k, int64_t nslabs, uint64_t* lists, hipStream_t stream) {
    const size_t lds = scan_lds_bytes(QB, M, ksub);
    const dim3 grid((unsigned)((n + QB - 1) / QB), (unsigned)nslabs);
    if (ksub == 256) {
        AT_RAISE_LDS(ctx, (pq_scan_kernel<QB, W, true>), lds);
        AT_LAUNCH((pq_scan_kernel<QB, W, true>), grid, dim3(WG), lds, stream, x, (long)n, d, M, ksub, cb, codes,
                  (long)ntotal, k, lists);
    } else {
        AT_RAISE_LDS(ctx, (pq_scan_kernel<QB, W, false>), lds);
        AT_LAUNCH((pq_scan_kernel<QB, W, false>), grid, dim3(WG), lds, stream, x, (long)n, d, M, ksub, cb, codes,
                  (long)ntotal, k, lists);
    }
    return AT_OK;
}

template <int QB>
int launch_scan_by_width(at_ctx* ctx, const float* x, int64_t n, int d, int M, int ksub, const float* cb,
                         const uint8_t* codes, int64_t ntotal, int k, int64_t nslabs, uint64_t* lists, hipStream_t stream) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(codes);
    if (M % 16 == 0 && a % 16 == 0) return launch_scan<QB, 16>(ctx, x, n, d, M, ksub, cb, codes, ntotal, k, nslabs, lists, stream);
    if (M % 8 == 0 && a % 8 == 0) return launch_scan<QB, 8>(ctx, x, n, d, M, ksub, cb, codes, ntotal, k, nslabs, lists, stream);
    if (M % 4 == 0 && a % 4 == 0) return launch_scan<QB, 4>(ctx, x, n, d, M, ksub, cb, codes, ntotal, k, nslabs, lists, stream);
    return launch_scan<QB, 1>(ctx, x, n, d, M, ksub, cb, codes, ntotal, k, nslabs, lists, stream);
}

}  // namespace

extern "C" int at_pq_search_limits(int* queries_per_block_out, int* slab_rows, int64_t* queries_per_chunk, int M,
                                   int64_t ntotal, int k) {
    AT_REQUIRE(M >= 1 && M <= MAX_M && k >= 1 && k <= MAX_K && ntotal >= 0 && ntotal < ((int64_t)1 << 31),
               "at_pq_search_limits: bad sizes M=%d ntotal=%lld k=%d", M, (long long)ntotal, k);
    const Plan p = make_plan(M, ntotal, k);
    if (queries_per_block_out) *queries_per_block_out = p.qb;
    if (slab_rows) *slab_rows = SLAB;
    if (queries_per_chunk) *queries_per_chunk = p.chunk;
    return AT_OK;
}

extern "C" int at_pq_search_f32(at_ctx* ctx, const float* x, int64_t n, int d, int M, int ksub, const float* codebooks,
                                const uint8_t* codes, int64_t ntotal, int k, int64_t* ids, float* dist, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_pq_search_f32: ctx is null");
    AT_REQUIRE(n >= 0 && d > 0 && M >= 1 && M <= MAX_M && d % M == 0 && ksub >= 1 && ksub <= 256 && k >= 1 && k <= MAX_K &&
                   ntotal >= 0 && ntotal < ((int64_t)1 << 31),
               "at_pq_search_f32: bad sizes n=%lld d=%d M=%d (1 .. %d) ksub=%d ntotal=%lld k=%d (1 .. %d)", (long long)n, d,
               M, MAX_M, ksub, (long long)ntotal, k, MAX_K);
    if (n == 0) return AT_OK;
    AT_REQUIRE(x && codebooks && ids && (codes || ntotal == 0), "at_pq_search_f32: null pointer");
    AT_REQUIRE(n <= ((int64_t)1 << 38) / (d > k ? d : k), "at_pq_search_f32: n=%lld too large", (long long)n);
    AT_HIP(hipSetDevice(ctx->device));
    if (ntotal == 0) {
        const int64_t total = n * k;
        AT_LAUNCH(pq_nothing_kernel, dim3((unsigned)((total + WG - 1) / WG)), dim3(WG), 0, stream, (long)total,
                  reinterpret_cast<long*>(ids), dist);
        return AT_OK;
    }

    const Plan p = make_plan(M, ntotal, k);
    const int64_t chunk = p.chunk < n ? p.chunk : n;
    int rc = at_guard_enter(&ctx->guard[AT_GUARD_PQ_SEARCH], stream);   // calls of one context share WS_PQ_SEARCH_LISTS
    if (rc) return rc;
    uint64_t* lists = static_cast<uint64_t*>(at_ws(ctx, WS_PQ_SEARCH_LISTS, p.per_query * (size_t)chunk, stream));
    if (!lists) return AT_E_NOMEM;
    for (int64_t q0 = 0; q0 < n; q0 += chunk) {
        const int64_t nq = n - q0 < chunk ? n - q0 : chunk;
        const float* xq = x + q0 * d;
        rc = p.qb == 4 ? launch_scan_by_width<4>(ctx, xq, nq, d, M, ksub, codebooks, codes, ntotal, k, p.nslabs, lists, stream)
                       : launch_scan_by_width<2>(ctx, xq, nq, d, M, ksub, codebooks, codes, ntotal, k, p.nslabs, lists, stream);
        if (rc) return rc;
        AT_LAUNCH(pq_merge_kernel, dim3((unsigned)nq), dim3(WG), 0, stream, lists, (long)(p.nslabs * k), k,
                  reinterpret_cast<long*>(ids + q0 * k), dist ? dist + q0 * k : nullptr);
    }
    return at_guard_leave(&ctx->guard[AT_GUARD_PQ_SEARCH], stream);
}
