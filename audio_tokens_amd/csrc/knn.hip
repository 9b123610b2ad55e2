// knn.hip -- the k nearest centroids under squared L2 on gfx950 (at_knn_f32, IndexFlatL2.search(x, k)).
//
// Arithmetic contract: dis(i,j) is at_assign_f32's value bit for bit (assign.hip, header):
//   ip, |x|^2, |c|^2 ascending fmaf chains (v_mfma_f32_32x32x2_f32), dis = (xn + cn) - 2*ip in one fma, then the
//   clamp v < 0 ? 0 : v, which leaves a NaN a NaN; n < 20: the direct form sum (x-c)^2.
// Listed: the k smallest finite (dis, j) in lexicographic order, ascending; the rest of a row is (-1, +inf).
//
// Fused path (2 <= k <= K_FUSED): the dense sweep over the chunked centroid image (chunked_sweep.h: the layout, the
// LDS-DMA stream, the x side and the MFMA block; x rows in registers at d = 64, 128, re-read one chunk per stage at any
// other d that is a multiple of 4), and what this kernel does with a finished tile: a running per-lane top-KL list
// (KL = the power of two >= k, at least 4) in registers (topk_lanes.h: the list, the pre-test and the merge, shared
// with ivf.hip).  A finished accumulator gives each lane 16 candidates; the
// wave first compares their minimum with every lane's KL-th key (one ballot) and then each candidate (one ballot
// each), so the insert network runs only for candidates that improve some lane.  A lane sees its centroids in
// ascending index order ((tile, accumulator, register) is ascending in j for a fixed half-wave), so a strict `<` insert that puts a candidate behind its equals keeps the
// lexicographic (dis, j) order without comparing ids.  The two half-waves (same 32 rows, disjoint centroids) merge
// once at the end: the elementwise (dis, j)-minimum of one list and the other reversed is a bitonic sequence of the
// KL smallest, sorted by a bitonic merge network.
//
// General path (k > K_FUSED, n < 20, and x without 16-byte rows or d % 4 != 0): blocks of rows x all centroids of
// keys (dis bits << idbits) | j in the context workspace (same sweep, keys written instead of a list; the direct /
// scalar-chain form for the other cases), a segmented rocPRIM radix sort per row, and the first k keys decoded.
// Non-finite distances get the all-ones key and are never listed.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "at_internal.h"
#include "chunked_sweep.h"
#include "topk_lanes.h"

namespace {

constexpr int WG = 256;        // 4 waves
constexpr int NA = 4;          // 32-centroid accumulators per tile (128 centroids)
constexpr int K_FUSED = 32;    // largest k of the fused path
constexpr int64_t ROWS_PER_LAUNCH = (int64_t)1 << 30;
constexpr size_t GENERAL_BYTES = (size_t)256 << 20;   // keys (in + out) of one block of the general path

// sort key of one distance: (bits << idbits) | j; non-finite -> all ones (sorts last, never listed)
__device__ __forceinline__ uint64_t dis_key(float v, unsigned j, int idbits, uint64_t none) {
    unsigned b = __float_as_uint(v);
    if (v == 0.0f) b = 0u;                       // -0 -> +0
    return b < 0x7f800000u ? (((uint64_t)b << idbits) | j) : none;
}

// MODE_TOPK: running top-KL per row, written as [n][k];  MODE_KEYS: every (row, centroid) key, [n][kc]
enum { MODE_TOPK = 0, MODE_KEYS = 1 };

// NCH > 0: d = 64 * NCH, x in registers; NCH = 0: any d % 4 == 0, x chunk re-read per stage
template <int NCH, int KL, int MODE, int WPS>
__global__ void __launch_bounds__(WG, WPS)
knn_mfma_kernel(const float* __restrict__ X, long n, int d, int nchunks, const float* __restrict__ img, int ntiles,
                int kc, int k, long* __restrict__ ids, float* __restrict__ dist, uint64_t* __restrict__ keys,
                int idbits) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 2 * cs::buf_floats(NA) floats
    cs::Sweep<NA, NCH, true> sweep(img, smem, nchunks, ntiles);
    const int j = sweep.j, h = sweep.h;
    const long row0 = ((long)blockIdx.x * 4 + sweep.wave) * 32;

    long r = row0 + j;
    if (r >= n) r = n - 1;
    const int dd = NCH > 0 ? NCH * cs::DC : d;
    const float* xrow = X + r * (long)dd;
    const float xn = cs::sqnorm16(xrow, dd);
    float xr[NCH > 0 ? NCH : 1][cs::DC / 2];
    if constexpr (NCH > 0) {
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) cs::load_x_chunk(xrow, ch, dd, h, xr[ch]);
    }

    float ld[KL];
    unsigned li[KL];
    tk::clear<KL>(ld, li);
    const long krow = row0 + j;                      // this lane's row (for the keys)
    const uint64_t none = idbits + 31 >= 64 ? ~0ull : ((1ull << (idbits + 31)) - 1ull);

    // The finished tile is handled inside the stage itself, not in a functor of cs::Sweep::run: with the top-k insert
    // network behind a call boundary the compiler spends up to 24 more registers on the same instructions.
    f32x16 acc[NA];
    auto stage = [&](int s, int ct, int ch, const float (&xv)[cs::DC / 2]) {
        const float* cur = sweep.begin_stage(smem, s, ct, ch);
        sweep.mfma_piece(acc, cur, xv, ch == 0);
        if (ch == sweep.nch - 1) {
            const float* cnorm = cur + sweep.PIECE_F;   // the tile's norms
#pragma unroll
            for (int a = 0; a < NA; a++) {
                const unsigned idbase = (unsigned)cs::acc_base(ct * NA + a, h);
                float u[16];
                tk::l2_of_acc16(acc[a], cnorm + a * 32 + 4 * h, xn, u);
                if constexpr (MODE == MODE_KEYS) {
                    if (krow < n) {
                        uint64_t* kr = keys + krow * (long)kc;
#pragma unroll
                        for (int e = 0; e < 16; e++) {
                            const unsigned id = idbase + (unsigned)cs::reg_offset(e);
                            if (id < (unsigned)kc) kr[id] = dis_key(cs::clamp0(u[e]), id, idbits, none);
                        }
                    }
                } else {
                    tk::offer16<KL>(ld, li, u, idbase);
                }
            }
        }
        __syncthreads();
    };
    sweep.prime();
    if constexpr (NCH > 0) {
        for (int ct = 0; ct < ntiles; ct++) {   // (written out: a chunk index must be a constant here)
            stage(ct * NCH, ct, 0, xr[0]);
            if constexpr (NCH == 2) stage(ct * NCH + 1, ct, 1, xr[NCH - 1]);
        }
    } else {
        int ct = 0, ch = 0;
        for (int s = 0; s < sweep.nstages; s++) {
            cs::load_x_chunk(xrow, ch, d, h, xr[0]);
            stage(s, ct, ch, xr[0]);
            if (++ch == sweep.nch) { ch = 0; ct++; }
        }
    }

    if constexpr (MODE == MODE_TOPK) {
        float cd[KL];
        unsigned ci[KL];
        tk::merge_halves<KL>(ld, li, cd, ci);
        if (h == 0 && krow < n) {
            long* io = ids + krow * (long)k;
            float* dout = dist ? dist + krow * (long)k : nullptr;
#pragma unroll
            for (int s = 0; s < KL; s++) {
                if (s < k) {
                    const bool has = ci[s] != cs::NONE;
                    io[s] = has ? (long)ci[s] : -1L;
                    if (dout) dout[s] = has ? cd[s] : __builtin_inff();
                }
            }
        }
    }
}

// The same keys without the MFMA sweep: n < 20 (faiss's direct form sum (x-c)^2) and rows the sweep cannot read
// (d % 4 != 0 or not 16-byte aligned: the three ascending scalar chains).  One thread per (row, centroid).
__global__ void __launch_bounds__(WG)
knn_keys_scalar_kernel(const float* __restrict__ X, long n, int d, const float* __restrict__ C, int kc, int direct,
                       uint64_t* __restrict__ keys, int idbits) {
    const long t = (long)blockIdx.x * WG + threadIdx.x;
    const long i = t / kc;
    const int c = (int)(t % kc);
    if (i >= n) return;
    const float* xi = X + i * d;
    const float* cc = C + (size_t)c * d;
    float v;
    if (direct) {
        float acc = 0.0f;
        for (int f = 0; f < d; f++) {
            const float df = xi[f] - cc[f];
            acc = __builtin_fmaf(df, df, acc);
        }
        v = acc;
    } else {
        float xn = 0.0f, cn = 0.0f, ip = 0.0f;
        for (int f = 0; f < d; f++) {
            xn = __builtin_fmaf(xi[f], xi[f], xn);
            cn = __builtin_fmaf(cc[f], cc[f], cn);
            ip = __builtin_fmaf(xi[f], cc[f], ip);
        }
        v = cs::clamp0(__builtin_fmaf(-2.0f, ip, xn + cn));
    }
    const uint64_t none = (1ull << (idbits + 31)) - 1ull;
    keys[t] = dis_key(v, (unsigned)c, idbits, none);
}

__global__ void __launch_bounds__(WG) knn_offsets_kernel(unsigned* __restrict__ off, int rows, int kc) {
    const int t = blockIdx.x * WG + threadIdx.x;
    if (t <= rows) off[t] = (unsigned)t * (unsigned)kc;
}

// first k keys of every sorted row -> (ids, dist); past kc or non-finite: (-1, +inf)
__global__ void __launch_bounds__(WG)
knn_decode_kernel(const uint64_t* __restrict__ sorted, long rows, int kc, int k, int idbits, long* __restrict__ ids,
                  float* __restrict__ dist) {
    const long t = (long)blockIdx.x * WG + threadIdx.x;
    if (t >= rows * (long)k) return;
    const long i = t / k;
    const int p = (int)(t % k);
    long id = -1;
    float dv = __builtin_inff();
    if (p < kc) {
        const uint64_t key = sorted[i * kc + p];
        const unsigned b = (unsigned)(key >> idbits);
        if (b < 0x7f800000u) {
            id = (long)(key & ((1ull << idbits) - 1ull));
            dv = __uint_as_float(b);
        }
    }
    ids[t] = id;
    if (dist) dist[t] = dv;
}

template <int NCH, int KL, int MODE, int WPS>
int launch_sweep(at_ctx* ctx, const float* x, int64_t n, int d, const float* img, int ntiles, int kc, int k,
                 int64_t* ids, float* dist, uint64_t* keys, int idbits, hipStream_t stream) {
    auto kern = &knn_mfma_kernel<NCH, KL, MODE, WPS>;
    const size_t lds = 2 * sizeof(float) * cs::buf_floats(NA);
    { const int rc = at_raise_lds(ctx, reinterpret_cast<const void*>(kern), lds); if (rc) return rc; }
    const int nchunks = cs::nchunks_of(d);
    for (int64_t r0 = 0; r0 < n; r0 += ROWS_PER_LAUNCH) {
        const int64_t m = n - r0 < ROWS_PER_LAUNCH ? n - r0 : ROWS_PER_LAUNCH;
        AT_LAUNCH(kern, dim3((unsigned)((m + 127) / 128)), dim3(WG), lds, stream, x + r0 * d, (long)m, d, nchunks, img,
                  ntiles, kc, k, ids ? reinterpret_cast<long*>(ids + r0 * k) : nullptr, dist ? dist + r0 * k : nullptr,
                  keys ? keys + r0 * kc : nullptr, idbits);
    }
    return AT_OK;
}

template <int KL>
int launch_fused(at_ctx* ctx, const float* x, int64_t n, int d, const float* img, int ntiles, int kc, int k,
                 int64_t* ids, float* dist, hipStream_t stream) {
    if (d == 64) return launch_sweep<1, KL, MODE_TOPK, 2>(ctx, x, n, d, img, ntiles, kc, k, ids, dist, nullptr, 0, stream);
    if (d == 128) return launch_sweep<2, KL, MODE_TOPK, 2>(ctx, x, n, d, img, ntiles, kc, k, ids, dist, nullptr, 0, stream);
    return launch_sweep<0, KL, MODE_TOPK, 2>(ctx, x, n, d, img, ntiles, kc, k, ids, dist, nullptr, 0, stream);
}

size_t knn_align(size_t b) { return (b + 255) & ~size_t(255); }

}  // namespace

extern "C" int at_knn_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int kc, int k, int64_t* ids,
                          float* dist, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_knn_f32: ctx is null");
    AT_REQUIRE(k >= 1, "at_knn_f32: k = %d (k must be at least 1)", k);
    AT_REQUIRE(n >= 0 && d > 0 && kc > 0 && kc <= (1 << 24), "at_knn_f32: bad sizes n=%lld d=%d k_c=%d", (long long)n,
               d, kc);
    if (n == 0) return AT_OK;
    AT_REQUIRE(x && c && ids, "at_knn_f32: null pointer");
    AT_HIP(hipSetDevice(ctx->device));

    // The workspace slots are the context's: a call on another stream than the previous one waits for it.
    { const int grc = at_guard_enter(&ctx->guard[AT_GUARD_KNN], stream); if (grc) return grc; }

    const bool sweep = n >= 20 && d % 4 == 0 && at_aligned16(x);
    int rc = AT_OK;
    int idbits = 1;
    while ((1 << idbits) < kc) idbits++;
    const int ntiles = (kc + cs::tile_rows(NA) - 1) / cs::tile_rows(NA);
    float* img = nullptr;
    if (sweep) {
        img = static_cast<float*>(at_ws(ctx, WS_KNN_IMG, sizeof(float) * ntiles * at_chunked_image_tile_floats(d, NA),
                                        stream));
        if (!img) return AT_E_NOMEM;
        rc = at_prep_chunked_image(ctx, c, kc, d, NA, img, stream);
        if (rc) return rc;
    }

    if (sweep && k <= K_FUSED) {
        if (k <= 4) rc = launch_fused<4>(ctx, x, n, d, img, ntiles, kc, k, ids, dist, stream);
        else if (k <= 8) rc = launch_fused<8>(ctx, x, n, d, img, ntiles, kc, k, ids, dist, stream);
        else if (k <= 16) rc = launch_fused<16>(ctx, x, n, d, img, ntiles, kc, k, ids, dist, stream);
        else rc = launch_fused<32>(ctx, x, n, d, img, ntiles, kc, k, ids, dist, stream);
    } else {
        // general path: blocks of rows, every key of a block sorted per row
        int64_t rows = (int64_t)(GENERAL_BYTES / (2 * sizeof(uint64_t) * (size_t)kc));
        if (rows < 1) rows = 1;
        if (rows > n) rows = n;
        const size_t nkeys = (size_t)rows * kc;
        size_t sort_bytes = 0;
        AT_HIP(rocprim::segmented_radix_sort_keys(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                  (unsigned)nkeys, (unsigned)rows, (const unsigned*)nullptr,
                                                  (const unsigned*)nullptr, 0, (unsigned)(idbits + 31), stream));
        const size_t b_keys = knn_align(8 * nkeys), b_off = knn_align(4 * (size_t)(rows + 1));
        unsigned char* w = static_cast<unsigned char*>(at_ws(ctx, WS_KNN, 2 * b_keys + b_off + knn_align(sort_bytes),
                                                             stream));
        if (!w) return AT_E_NOMEM;
        uint64_t* kin = reinterpret_cast<uint64_t*>(w);
        uint64_t* kout = reinterpret_cast<uint64_t*>(w + b_keys);
        unsigned* off = reinterpret_cast<unsigned*>(w + 2 * b_keys);
        void* tmp = w + 2 * b_keys + b_off;
        AT_LAUNCH(knn_offsets_kernel, dim3((unsigned)((rows + WG) / WG)), dim3(WG), 0, stream, off, (int)rows, kc);
        for (int64_t r0 = 0; r0 < n && rc == AT_OK; r0 += rows) {
            const int64_t m = n - r0 < rows ? n - r0 : rows;
            const float* xb = x + r0 * d;
            if (sweep) {
                if (d == 64) rc = launch_sweep<1, 4, MODE_KEYS, 2>(ctx, xb, m, d, img, ntiles, kc, k, nullptr, nullptr, kin, idbits, stream);
                else if (d == 128) rc = launch_sweep<2, 4, MODE_KEYS, 2>(ctx, xb, m, d, img, ntiles, kc, k, nullptr, nullptr, kin, idbits, stream);
                else rc = launch_sweep<0, 4, MODE_KEYS, 2>(ctx, xb, m, d, img, ntiles, kc, k, nullptr, nullptr, kin, idbits, stream);
                if (rc) break;
            } else {
                AT_LAUNCH(knn_keys_scalar_kernel, dim3((unsigned)((m * kc + WG - 1) / WG)), dim3(WG), 0, stream, xb,
                          (long)m, d, c, kc, n < 20 ? 1 : 0, kin, idbits);
            }
            size_t sb = sort_bytes;
            AT_HIP(rocprim::segmented_radix_sort_keys(tmp, sb, (const uint64_t*)kin, kout, (unsigned)(m * kc),
                                                      (unsigned)m, (const unsigned*)off, (const unsigned*)off + 1, 0,
                                                      (unsigned)(idbits + 31), stream));
            AT_LAUNCH(knn_decode_kernel, dim3((unsigned)((m * k + WG - 1) / WG)), dim3(WG), 0, stream, kout, (long)m,
                      kc, k, idbits, reinterpret_cast<long*>(ids + r0 * k), dist ? dist + r0 * k : nullptr);
        }
    }
    // behind everything this call queued: a later call on another stream waits for it
    { const int grc = at_guard_leave(&ctx->guard[AT_GUARD_KNN], stream); if (grc) return grc; }
    return rc;
}
