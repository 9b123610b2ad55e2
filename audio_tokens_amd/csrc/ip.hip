// ip.hip -- the centroid with the largest inner product on gfx950 (at_assign_ip_f32, IndexFlatIP.search(x, 1)) and the
// per-row re-normalisation of spherical k-means (at_renorm_rows_f32, faiss fvec_renorm_L2).
//
// Arithmetic contract of the search:
//   ip(i,j) = fmaf chain over the feature index, ascending, from +0 (v_mfma_f32_32x32x2_f32): the ip of at_assign_f32,
//             at every n (faiss's small-batch form is the same sum);
//   centroid j is listed for row i iff ip(i,j) > -inf (a NaN product never is, +inf is);
//   ids[i] = the lowest j among the listed centroids with the largest ip(i,j), ip[i] = that product with its own bits;
//   rows with nothing to list: ids = -1, ip = -inf.
//
// Sweep (d % 4 == 0, 16-byte aligned rows): the dense sweep of knn.hip with its per-lane top-k list replaced by a running
// best.  Centroids are staged through double-buffered LDS by LDS-DMA from the chunked centroid image (assign.hip,
// at_prep_chunked_image: tiles of 128 rows, 64 features per chunk); x rows stay in registers (d = 64, 128: one / two
// chunks, template specialisations) or are re-read from L2 one chunk per stage (any other d).  The 32x32 accumulator
// puts the x row on the lane and 16 centroids in its registers, and a lane sees its centroids in ascending index order
// ((tile, accumulator, register) is ascending in j for a fixed half-wave), so a strict `>` keeps the lowest index without
// comparing ids; the two half-waves (same 32 rows, disjoint centroids) merge once at the end, the lower index winning
// on equal products.  There is no |x|^2 + |c|^2 epilogue, and the norms behind a tile of the image are not read: a
// zero-filled pad row would score +0 and beat every negative product, so the rows >= k of the last tile are masked by
// their index (a norm of +inf marks pad rows in the L2 sweeps, but a real centroid's norm may overflow to it as well).
//
// Everything else (d % 4 != 0, rows that are not 16-byte aligned): the same chain in scalar code, one thread per row.
#include "at_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int WG = 256;        // 4 waves
constexpr int DC = 64;         // features per chunk of the centroid image
constexpr int NA = 4;          // 32-centroid accumulators per tile (128 centroids)
constexpr unsigned NONE = 0xffffffffu;

__device__ __forceinline__ void dma_1k(const float* gsrc_lane, float* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc_lane,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// NCH > 0: d = 64 * NCH, x in registers; NCH = 0: any d % 4 == 0, x chunk re-read per stage
template <int NCH>
__global__ void __launch_bounds__(WG, 2)
ip_mfma_kernel(const float* __restrict__ X, long n, int d, int nchunks, const float* __restrict__ img, size_t tile_f,
               int ntiles, int kc, long* __restrict__ ids, float* __restrict__ ipo) {
    constexpr int R = 32 * NA;
    constexpr int PIECE_F = R * DC;
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 2 * PIECE_F floats

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31;   // x row within the wave's 32 rows == accumulator column
    const int h = lane >> 5;   // which k of each MFMA k-pair this lane feeds
    const long row0 = ((long)blockIdx.x * 4 + wave) * 32;
    const int nch = NCH > 0 ? NCH : nchunks;

    long r = row0 + j;
    if (r >= n) r = n - 1;
    const float* xrow = X + r * (long)(NCH > 0 ? NCH * DC : d);
    float xr[NCH > 0 ? NCH : 1][DC / 2];
    auto load_x = [&](int chx, float (&xv)[DC / 2], int dd) {
#pragma unroll
        for (int q = 0; q < DC / 8; q++) {
            const int f = chx * DC + 8 * q;
            f32x4 u = {0, 0, 0, 0}, v = {0, 0, 0, 0};
            if (f < dd) u = *reinterpret_cast<const f32x4*>(xrow + f);          // dd % 4 == 0
            if (f + 4 < dd) v = *reinterpret_cast<const f32x4*>(xrow + f + 4);
            xv[4 * q + 0] = h ? u[1] : u[0];
            xv[4 * q + 1] = h ? u[3] : u[2];
            xv[4 * q + 2] = h ? v[1] : v[0];
            xv[4 * q + 3] = h ? v[3] : v[2];
        }
    };
    if constexpr (NCH > 0) {
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) load_x(ch, xr[ch], NCH * DC);
    }

    // running best of this lane: the product and the code (tile * NA + accumulator) * 16 + register of its centroid
    float best = -__builtin_inff();
    unsigned bcode = NONE;

    auto stage_dma = [&](int ct, int ch, float* dst) {
        const float* src = img + (size_t)ct * tile_f + (size_t)ch * PIECE_F;
        for (int p = wave; p < PIECE_F / 256; p += 4) dma_1k(src + p * 256 + lane * 4, dst + p * 256);
    };
    stage_dma(0, 0, smem);
    __syncthreads();

    const int swz = j & 15;
    const int nstages = ntiles * nch;
    f32x16 acc[NA];
    auto stage = [&](int s, int ct, int ch, const float (&xv)[DC / 2]) {
        const float* cur = smem + (s & 1) * PIECE_F;
        if (s + 1 < nstages) {
            const bool wrap = ch + 1 == nch;
            stage_dma(wrap ? ct + 1 : ct, wrap ? 0 : ch + 1, smem + ((s + 1) & 1) * PIECE_F);
        }
#pragma unroll
        for (int a = 0; a < NA; a++) {
            const float* arow = cur + (a * 32 + j) * DC;
            f32x16 cacc = acc[a];
            if (ch == 0) cacc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < DC / 8; q++) {
                const int pc = (2 * q + h) ^ swz;
                const f32x4 av = *reinterpret_cast<const f32x4*>(arow + pc * 4);
                cacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], xv[4 * q + 0], cacc, 0, 0, 0);
                cacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], xv[4 * q + 1], cacc, 0, 0, 0);
                cacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], xv[4 * q + 2], cacc, 0, 0, 0);
                cacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], xv[4 * q + 3], cacc, 0, 0, 0);
            }
            acc[a] = cacc;
        }
        if (ch == nch - 1) {
            // accumulator register e holds centroid (ct * NA + a) * 32 + 4 * h + (e & 3) + 8 * (e >> 2): ascending in e
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
                    const int idbase = (ct * NA + a) * 32 + 4 * h;
#pragma unroll
                    for (int e = 0; e < 16; e++) {
                        const bool gt = acc[a][e] > best && idbase + (e & 3) + 8 * (e >> 2) < kc;
                        best = gt ? acc[a][e] : best;
                        bcode = gt ? codebase + (unsigned)e : bcode;
                    }
                }
            }
        }
        __syncthreads();
    };

    if constexpr (NCH > 0) {
        static_assert(NCH <= 2, "x chunks held in registers: d = 64 or 128");
        for (int ct = 0; ct < ntiles; ct++) {   // (written out: a chunk index must be a constant here)
            stage(ct * NCH, ct, 0, xr[0]);
            if constexpr (NCH == 2) stage(ct * NCH + 1, ct, 1, xr[NCH - 1]);
        }
    } else {
        int ct = 0, ch = 0;
        for (int s = 0; s < nstages; s++) {
            load_x(ch, xr[0], d);
            stage(s, ct, ch, xr[0]);
            if (++ch == nch) { ch = 0; ct++; }
        }
    }

    // merge the half-waves: the larger product, the lower index on equal products (NONE is the highest index)
    unsigned idx = NONE;
    if (bcode != NONE) {
        const unsigned e = bcode & 15u;
        idx = (bcode >> 4) * 32u + (e & 3u) + 8u * (e >> 2) + 4u * (unsigned)h;
    }
    const float ov = __shfl_xor(best, 32);
    const unsigned oi = (unsigned)__shfl_xor((int)idx, 32);
    if (ov > best || (ov == best && oi < idx)) {
        best = ov;
        idx = oi;
    }
    const long ro = row0 + j;
    if (h == 0 && ro < n) {
        ids[ro] = idx == NONE ? -1L : (long)idx;
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
    const int ntiles = (kc + 32 * NA - 1) / (32 * NA);
    const size_t tile_f = at_chunked_image_tile_floats(d, NA);
    float* img = static_cast<float*>(at_ws(ctx, WS_IP_IMG, sizeof(float) * ntiles * tile_f, stream));
    if (!img) return AT_E_NOMEM;
    { const int rc = at_prep_chunked_image(ctx, c, kc, d, NA, img, stream); if (rc) return rc; }
    const size_t lds = 2 * sizeof(float) * 32 * NA * DC;
    AT_RAISE_LDS(ctx, ip_mfma_kernel<NCH>, lds);
    AT_LAUNCH(ip_mfma_kernel<NCH>, dim3((unsigned)((n + 127) / 128)), dim3(WG), lds, stream, x, (long)n, d,
              (d + DC - 1) / DC, img, tile_f, ntiles, kc, reinterpret_cast<long*>(ids), ipo);
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
        if (d == 64) return launch_ip_sweep<1>(ctx, x, n, d, c, k, ids, ip, stream);
        if (d == 128) return launch_ip_sweep<2>(ctx, x, n, d, c, k, ids, ip, stream);
        return launch_ip_sweep<0>(ctx, x, n, d, c, k, ids, ip, stream);
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
