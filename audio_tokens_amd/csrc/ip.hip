// ip.hip -- the centroid with the largest inner product on gfx950 (at_assign_ip_f32, IndexFlatIP.search(x, 1)) and the
// per-row re-normalisation of spherical k-means (at_renorm_rows_f32, faiss fvec_renorm_L2).
//
// Arithmetic contract of the search:
//   ip(i,j) = fmaf chain over the feature index, ascending, from +0 (v_mfma_f32_32x32x2_f32): the ip of at_assign_f32,
//             at every n (faiss's small-batch form is the same sum); a zero result keeps the sign the chain gives it (a
//             negative product that underflows rounds to -0), at every d;
//   centroid j is listed for row i iff ip(i,j) > -inf (a NaN product never is, +inf is);
//   ids[i] = the lowest j among the listed centroids with the largest ip(i,j), ip[i] = that product with its own bits;
//   rows with nothing to list: ids = -1, ip = -inf.
//
// Sweep (d % 4 == 0, 16-byte aligned rows): the dense sweep over the chunked centroid image (chunked_sweep.h: the
// layout, the LDS-DMA stream, the x side and the MFMA block; x rows in registers at d = 64, 128, re-read one chunk per
// stage at any other d), and what this kernel does with a finished tile: a running best.  The 32x32 accumulator
// puts the x row on the lane and 16 centroids in its registers, and a lane sees its centroids in ascending index order
// ((tile, accumulator, register) is ascending in j for a fixed half-wave), so a strict `>` keeps the lowest index
// without comparing ids; the two half-waves (same 32 rows, disjoint centroids) merge once at the end, the lower index
// winning on equal products.  There is no |x|^2 + |c|^2 epilogue, and the norms behind a tile of the image are not read: a
// zero-filled pad row would score +0 and beat every negative product, so the rows >= k of the last tile are masked by
// their index (a norm of +inf marks pad rows in the L2 sweeps, but a real centroid's norm may overflow to it as well).
// Calls of one context share the image's slot, WS_IP_IMG: a call on another stream than the previous one waits for it.
//
// Everything else (d % 4 != 0, rows that are not 16-byte aligned): the same chain in scalar code, one thread per row.
#include "at_internal.h"
#include "chunked_sweep.h"

namespace {

constexpr int WG = 256;        // 4 waves
constexpr int NA = 4;          // 32-centroid accumulators per tile (128 centroids)

// NCH > 0: d = 64 * NCH, x in registers; NCH = 0: any d % 4 == 0, x chunk re-read per stage
template <int NCH>
__global__ void __launch_bounds__(WG, 2)
ip_mfma_kernel(const float* __restrict__ X, long n, int d, int nchunks, const float* __restrict__ img, int ntiles,
               int kc, long* __restrict__ ids, float* __restrict__ ipo) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 2 * cs::piece_floats(NA) floats
    cs::Sweep<NA, NCH, false> sweep(img, smem, nchunks, ntiles);
    const int j = sweep.j, h = sweep.h;
    const long row0 = ((long)blockIdx.x * 4 + sweep.wave) * 32;

    long r = row0 + j;
    if (r >= n) r = n - 1;
    const int dd = NCH > 0 ? NCH * cs::DC : d;
    const float* xrow = X + r * (long)dd;
    float xr[NCH > 0 ? NCH : 1][cs::DC / 2];
    if constexpr (NCH > 0) {
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) cs::load_x_chunk(xrow, ch, dd, h, xr[ch]);
    }

    // running best of this lane: the product and the code (tile * NA + accumulator) * 16 + register of its centroid
    float best = -__builtin_inff();
    unsigned bcode = cs::NONE;

    f32x16 acc[NA];
    sweep.prime();
    sweep.run(0, ntiles, acc, xr, xrow, d, [&](int ct, const float*, const f32x16 (&acc)[NA]) {
        if (ct + 1 < ntiles) {
#pragma unroll
            for (int a = 0; a < NA; a++) {
                const unsigned codebase = (unsigned)(ct * NA + a) * 16u;
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const bool gt = acc[a][e] > best;        // false for a NaN product, and for -inf
                    best = gt ? acc[a][e] : best;
                    bcode = gt ? codebase + (unsigned)e : bcode;
                }
            }
        } else {   // the last tile: its rows >= kc are padding
#pragma unroll
            for (int a = 0; a < NA; a++) {
                const unsigned codebase = (unsigned)(ct * NA + a) * 16u;
                const int idbase = cs::acc_base(ct * NA + a, h);
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const bool gt = acc[a][e] > best && idbase + cs::reg_offset(e) < kc;
                    best = gt ? acc[a][e] : best;
                    bcode = gt ? codebase + (unsigned)e : bcode;
                }
            }
        }
    }, -0.0f);   // the features behind d of a partial last chunk: a product of -0 keeps the chain's zero, sign included

    unsigned idx = cs::index_of(bcode, h);
    cs::merge_halves_max(best, idx);
    const long ro = row0 + j;
    if (h == 0 && ro < n) {
        ids[ro] = idx == cs::NONE ? -1L : (long)idx;
        if (ipo) ipo[ro] = best;
    }
}

// The same chain and the same listing rule in scalar code, one thread per row: any d, any alignment.
__global__ void __launch_bounds__(WG)
ip_scalar_kernel(const float* __restrict__ X, long n, int d, const float* __restrict__ C, int kc,
                 long* __restrict__ ids, float* __restrict__ ipo) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const float* xi = X + i * d;
    float best = -__builtin_inff();
    long bi = -1;
    for (int c = 0; c < kc; c++) {
        const float* cc = C + (size_t)c * d;
        float ip = 0.0f;
        for (int f = 0; f < d; f++) ip = __builtin_fmaf(xi[f], cc[f], ip);
        if (ip > best) {
            best = ip;
            bi = c;
        }
    }
    ids[i] = bi;
    if (ipo) ipo[i] = best;
}

// One wave per row.  Every lane walks the whole squared-norm chain (it is sequential by contract; the loads are
// broadcasts), then the lanes share the scaling.  The wave has read the whole row before any lane stores into it.
__global__ void __launch_bounds__(64) renorm_rows_kernel(float* __restrict__ C, int d) {
    float* row = C + (size_t)blockIdx.x * d;
    float nr = 0.0f;
    for (int f = 0; f < d; f++) nr = __builtin_fmaf(row[f], row[f], nr);
    if (!(nr > 0.0f)) return;                       // a zero row, or one that holds a NaN: left as it is
    const float inv = 1.0f / __builtin_sqrtf(nr);   // both correctly rounded (l2norm_core.h); +inf gives 0
    for (int f = threadIdx.x; f < d; f += 64) row[f] = row[f] * inv;
}

template <int NCH>
int launch_ip_sweep(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int kc, int64_t* ids, float* ipo,
                    hipStream_t stream) {
    const int ntiles = (kc + cs::tile_rows(NA) - 1) / cs::tile_rows(NA);
    float* img = static_cast<float*>(at_ws(ctx, WS_IP_IMG, sizeof(float) * ntiles * at_chunked_image_tile_floats(d, NA),
                                           stream));
    if (!img) return AT_E_NOMEM;
    { const int rc = at_prep_chunked_image(ctx, c, kc, d, NA, img, stream); if (rc) return rc; }
    const size_t lds = 2 * sizeof(float) * cs::piece_floats(NA);
    AT_RAISE_LDS(ctx, ip_mfma_kernel<NCH>, lds);
    AT_LAUNCH(ip_mfma_kernel<NCH>, dim3((unsigned)((n + 127) / 128)), dim3(WG), lds, stream, x, (long)n, d,
              cs::nchunks_of(d), img, ntiles, kc, reinterpret_cast<long*>(ids), ipo);
    return AT_OK;
}

}  // namespace

extern "C" int at_assign_ip_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k, int64_t* ids,
                                float* ip, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_assign_ip_f32: ctx is null");
    AT_REQUIRE(n >= 0 && d > 0 && k > 0, "at_assign_ip_f32: bad sizes n=%lld d=%d k=%d", (long long)n, d, k);
    if (n == 0) return AT_OK;
    AT_REQUIRE(x && c && ids, "at_assign_ip_f32: null pointer");
    AT_REQUIRE(k <= (1 << 24), "at_assign_ip_f32: k=%d too large", k);
    AT_REQUIRE(n <= ((int64_t)1 << 37), "at_assign_ip_f32: n=%lld too large", (long long)n);
    AT_HIP(hipSetDevice(ctx->device));

    if (d % 4 == 0 && at_aligned16(x)) {
        // calls of one context share WS_IP_IMG: a call on another stream than the previous one waits for it
        int rc = at_guard_enter(&ctx->guard[AT_GUARD_IP], stream);
        if (rc) return rc;
        if (d == 64) rc = launch_ip_sweep<1>(ctx, x, n, d, c, k, ids, ip, stream);
        else if (d == 128) rc = launch_ip_sweep<2>(ctx, x, n, d, c, k, ids, ip, stream);
        else rc = launch_ip_sweep<0>(ctx, x, n, d, c, k, ids, ip, stream);
        // behind everything this call queued, also where a later step failed
        const int grc = at_guard_leave(&ctx->guard[AT_GUARD_IP], stream);
        return rc ? rc : grc;
    }
    AT_LAUNCH(ip_scalar_kernel, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, stream, x, (long)n, d, c, k,
              reinterpret_cast<long*>(ids), ip);
    return AT_OK;
}

extern "C" int at_renorm_rows_f32(at_ctx* ctx, float* c, int64_t k, int d, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_renorm_rows_f32: ctx is null");
    AT_REQUIRE(k >= 0 && k <= 0x7fffffffLL && d > 0, "at_renorm_rows_f32: bad sizes k=%lld d=%d", (long long)k, d);
    if (k == 0) return AT_OK;
    AT_REQUIRE(c, "at_renorm_rows_f32: null pointer");
    AT_HIP(hipSetDevice(ctx->device));
    AT_LAUNCH(renorm_rows_kernel, dim3((unsigned)k), dim3(64), 0, stream, c, d);
    return AT_OK;
}
