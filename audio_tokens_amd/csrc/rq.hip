// rq.hip -- greedy residual quantiser on gfx950: at_rq_encode_f32 (ResidualQuantizer.compute_codes) and at_rq_decode_f32.
//
// r_0 = x.  Stage m = 0 .. M-1 quantises the running residual r_m against codebook m (ksub rows of d features):
// (codes[i][m], dist[i][m]) is at_assign_f32's answer for the rows r_m, bit for bit (assign.hip, header): ip, |r|^2,
// |c|^2 ascending fmaf chains over the d features from +0, dis = fma(-2, ip, rn + cn), the clamp v < 0 ? 0 : v (a NaN
// stays a NaN), the lowest index among equal distances; calls with n < 20 rows use the direct form sum (r-c)^2.  A row
// with no distance below +inf at a stage gets code 0, distance +inf, and raises *bad.  Then
// r_{m+1}[i][f] = r_m[i][f] - codebooks[m][codes[i][m]][f], one fp32 subtraction (a flagged row subtracts row 0).
//
// Fused path (d = 64 or 128, 16-byte aligned rows, codebooks and residual, n >= 20): one launch for all M stages.  The
// codebooks are prepared once per call into the chunked centroid image (chunked_sweep.h; at_prep_chunked_image: tiles
// of 128 rows, 64 features per chunk, |c|^2 of a tile behind its last chunk, +inf for pad rows, so ksub < 256 needs no
// masking) in WS_RQ_IMG: stage m owns the tiles m * tps .. m * tps + tps - 1, tps = ceil(ksub / 128) -- at ksub = 256
// the [M * 256][d] table is one image.  A wave owns 32 rows and the four waves of a workgroup share the tiles, which
// stream through double-buffered LDS by LDS-DMA (cs::Sweep, chunked_sweep.h); the piece behind the last one of stage m
// is the first of stage m + 1, so the stream never stalls on the residual update.
// Per stage: v_mfma_f32_32x32x2_f32 over the features in ascending order (the chain of the contract), the
// fma(-2, acc, rn + cn) epilogue with the clamp, a running strict `<` minimum over centroids met in ascending index
// ((tile, accumulator, register) ascends for a fixed half-wave), one merge of the two half-waves (same rows, disjoint
// centroids), the lower index winning on equal distances.  The winner's codebook row is then gathered with 16-byte
// loads (L2 hits) and subtracted in registers.  In the MFMA operand layout a lane holds the features of its row with
// the parity of its half-wave (register i: feature 2 i + h); |r|^2 of the new residual is the ascending chain over ALL
// d features, so the two half-waves exchange their new values once per stage (d / 2 cross-lane moves against
// 8 * d / 2 MFMAs of 16 passes) and both walk the whole chain.  x is read from HBM once; codes leave as one 32-bit
// store per four stages where M and the pointer allow, the residual is written only if asked for.
//
// General path (everything else): the same chains in scalar code, one launch.  A workgroup owns 8 rows for all M
// stages and each of its threads one word of the stage's codebook; the residual lives in the caller's buffer or in
// WS_RQ_TMP.  (Not a composition of at_assign_f32 calls: its kernels clamp with fmaxf, which turns a NaN distance into
// 0, so a row that holds a NaN would be given word 0 at distance 0 there instead of the flag.)
// Decode: out = codebooks[0][codes[.][0]], then + codebooks[m][codes[.][m]] for m = 1 .. M-1 in ascending order, one
// fp32 addition each; 16 bytes per thread where d and the pointers allow.  A code >= ksub makes the row NaN.
#include "at_internal.h"
#include "chunked_sweep.h"

namespace {

constexpr int WG = 256;        // 4 waves
constexpr int NA = 4;          // 32-centroid accumulators per tile (128 centroids)
using cs::clamp0;
using cs::NONE;

// d = 64 * NCH; tps tiles of the image per stage
template <int NCH>
__global__ void __launch_bounds__(WG, 2)
rq_fused_kernel(const float* __restrict__ X, long n, int M, int ksub, int tps, const float* __restrict__ img,
                const float* __restrict__ cb, uint8_t* __restrict__ codes, float* __restrict__ dist,
                float* __restrict__ resid, int* __restrict__ bad, int pack4) {
    constexpr int DC = cs::DC;
    constexpr int D = NCH * DC;
    static_assert(NCH == 1 || NCH == 2, "the residual stays in registers: d = 64 or 128");
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 2 * cs::buf_floats(NA) floats
    // the tiles of all stages are contiguous in the image: one stream, stage m its tiles m * tps .. m * tps + tps - 1
    cs::Sweep<NA, NCH, true> sweep(img, smem, NCH, M * tps);
    const int j = sweep.j, h = sweep.h;
    const long ro = ((long)blockIdx.x * 4 + sweep.wave) * 32 + j;
    const long r = ro < n ? ro : n - 1;
    const bool store = h == 0 && ro < n;

    // the residual: register i of chunk ch holds feature 64 ch + 2 i + h; rn its |r|^2 chain over all D features
    const float* xrow = X + r * (long)D;
    float xr[NCH][DC / 2];
    float rn = cs::sqnorm16(xrow, D);
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) cs::load_x_chunk(xrow, ch, D, h, xr[ch]);

    sweep.prime();
    const cs::CodeSink sink{codes, dist, bad, pack4};
    f32x16 acc[NA];
    unsigned pack = 0;
#pragma unroll 1
    for (int m = 0; m < M; m++) {
        float best = __builtin_inff();
        unsigned bcode = cs::NONE;   // (tile of the stage * NA + accumulator) * 16 + register
        const int t0 = m * tps;
        sweep.run(t0, t0 + tps, acc, xr, xrow, D, [&](int ct, const float* cnorm, const f32x16 (&acc)[NA]) {
            const float* cnh = cnorm + 4 * h;   // the norms of this half-wave's centroids
#pragma unroll
            for (int a = 0; a < NA; a++)
                cs::min16(acc[a], cnh + a * 32, rn, (unsigned)((ct - t0) * NA + a) * 16u, best, bcode);
        });
        const unsigned win = cs::merged_index(best, bcode, h);
        const unsigned idx = sink.put(win, best, store, ro * (long)M + m, m, pack);
        if (m + 1 == M && !resid) break;

        // r <- r - word (idx < ksub: a pad row's +inf norm never wins), and the |r|^2 chain of the new residual
        const float* crow = cb + ((size_t)m * ksub + idx) * D;
        rn = 0.0f;
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) {
#pragma unroll
            for (int q = 0; q < DC / 8; q++) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(crow + ch * DC + 8 * q);
                const f32x4 v = *reinterpret_cast<const f32x4*>(crow + ch * DC + 8 * q + 4);
                xr[ch][4 * q + 0] = xr[ch][4 * q + 0] - (h ? u[1] : u[0]);
                xr[ch][4 * q + 1] = xr[ch][4 * q + 1] - (h ? u[3] : u[2]);
                xr[ch][4 * q + 2] = xr[ch][4 * q + 2] - (h ? v[1] : v[0]);
                xr[ch][4 * q + 3] = xr[ch][4 * q + 3] - (h ? v[3] : v[2]);
            }
#pragma unroll
            for (int i = 0; i < DC / 2; i++) {
                const float mine = xr[ch][i];
                const float other = __shfl_xor(mine, 32);
                const float ev = h ? other : mine, od = h ? mine : other;   // features 2 i and 2 i + 1 of the chunk
                rn = __builtin_fmaf(ev, ev, rn);
                rn = __builtin_fmaf(od, od, rn);
            }
        }
    }

    if (resid) {
        // half-wave 0 stores the features 8 q .. 8 q + 3 of a row, half-wave 1 the features 8 q + 4 .. 8 q + 7
        float* out = resid + r * (long)D;
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) {
#pragma unroll
            for (int q = 0; q < DC / 8; q++) {
                const float a0 = xr[ch][4 * q + 0], a1 = xr[ch][4 * q + 1], a2 = xr[ch][4 * q + 2], a3 = xr[ch][4 * q + 3];
                const float r0 = __shfl_xor(h ? a0 : a2, 32);
                const float r1 = __shfl_xor(h ? a1 : a3, 32);
                const f32x4 w = h ? f32x4{r0, a2, r1, a3} : f32x4{a0, r0, a1, r1};
                if (ro < n) *reinterpret_cast<f32x4*>(out + ch * DC + 8 * q + 4 * h) = w;
            }
        }
    }
}

// General path: any d, any alignment, any ksub <= 256; direct: the call has n < 20 rows.  A workgroup owns RB rows for
// all M stages; thread w owns word w of the stage's codebook and walks the d features once for all RB rows (the rows'
// values are wave-wide broadcasts).  The residual lives in `res` (the caller's buffer or WS_RQ_TMP), touched by this
// workgroup alone: the barriers between the phases order its stores and loads.
constexpr int RB = 8;

__global__ void __launch_bounds__(WG)
rq_general_kernel(const float* __restrict__ X, long n, int d, int M, int ksub, const float* __restrict__ cb, int direct,
                  float* __restrict__ res, uint8_t* __restrict__ codes, float* __restrict__ dist, int* __restrict__ bad) {
    __shared__ float s_rn[RB];
    __shared__ float s_v[4][RB];
    __shared__ unsigned s_i[4][RB];
    __shared__ unsigned s_win[RB];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.x * RB;
    const int nb = n - row0 < RB ? (int)(n - row0) : RB;
    for (long e = tid; e < (long)nb * d; e += WG) res[row0 * d + e] = X[row0 * d + e];
    __syncthreads();
    const float* rrow[RB];   // (the slots behind the last row alias it: computed, never stored)
#pragma unroll
    for (int b = 0; b < RB; b++) rrow[b] = res + (row0 + (b < nb ? b : nb - 1)) * d;

    for (int m = 0; m < M; m++) {
        const float* book = cb + (size_t)m * ksub * d;
        if (!direct && tid < RB) {
            float rn = 0.0f;
            for (int f = 0; f < d; f++) rn = __builtin_fmaf(rrow[tid][f], rrow[tid][f], rn);
            s_rn[tid] = rn;
        }
        __syncthreads();
        float v[RB];
#pragma unroll
        for (int b = 0; b < RB; b++) v[b] = __builtin_inff();
        if (tid < ksub) {
            const float* cw = book + (size_t)tid * d;
            float acc[RB];
#pragma unroll
            for (int b = 0; b < RB; b++) acc[b] = 0.0f;
            if (direct) {
                for (int f = 0; f < d; f++) {
                    const float cf = cw[f];
#pragma unroll
                    for (int b = 0; b < RB; b++) {
                        const float df = rrow[b][f] - cf;
                        acc[b] = __builtin_fmaf(df, df, acc[b]);
                    }
                }
#pragma unroll
                for (int b = 0; b < RB; b++) v[b] = acc[b];
            } else {
                float cn = 0.0f;
                for (int f = 0; f < d; f++) {
                    const float cf = cw[f];
                    cn = __builtin_fmaf(cf, cf, cn);
#pragma unroll
                    for (int b = 0; b < RB; b++) acc[b] = __builtin_fmaf(rrow[b][f], cf, acc[b]);
                }
#pragma unroll
                for (int b = 0; b < RB; b++) v[b] = clamp0(__builtin_fmaf(-2.0f, acc[b], s_rn[b] + cn));
            }
        }
        // arg-min per row over the words: the smaller distance, the lower index on equal distances; a distance that
        // is not below +inf (a NaN, +inf) is never listed
#pragma unroll
        for (int b = 0; b < RB; b++) {
            const bool listed = v[b] < __builtin_inff();
            float bv = listed ? v[b] : __builtin_inff();
            unsigned bi = listed ? (unsigned)tid : NONE;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float ov = __shfl_xor(bv, o);
                const unsigned oi = (unsigned)__shfl_xor((int)bi, o);
                if (ov < bv || (ov == bv && oi < bi)) {
                    bv = ov;
                    bi = oi;
                }
            }
            if (lane == 0) {
                s_v[wave][b] = bv;
                s_i[wave][b] = bi;
            }
        }
        __syncthreads();
        if (tid < RB) {
            float bv = s_v[0][tid];
            unsigned bi = s_i[0][tid];
            for (int w = 1; w < 4; w++) {
                const float ov = s_v[w][tid];
                const unsigned oi = s_i[w][tid];
                if (ov < bv || (ov == bv && oi < bi)) {
                    bv = ov;
                    bi = oi;
                }
            }
            const bool none = bi == NONE;
            if (none) bi = 0u;
            s_win[tid] = bi;
            if (tid < nb) {
                const long o = (row0 + tid) * (long)M + m;
                codes[o] = (uint8_t)bi;
                if (dist) dist[o] = bv;
                if (none && bad) *bad = 1;
            }
        }
        __syncthreads();
        for (long e = tid; e < (long)nb * d; e += WG) {
            const int b = (int)(e / d);
            const int f = (int)(e % d);
            res[row0 * d + e] = res[row0 * d + e] - book[(size_t)s_win[b] * d + f];
        }
        __syncthreads();
    }
}

// 16 bytes per thread: d % 4 == 0, codebooks and out 16-byte aligned
__global__ void __launch_bounds__(WG)
rq_decode_vec_kernel(const uint8_t* __restrict__ codes, long n, int d, int M, int ksub, const float* __restrict__ cb,
                     float* __restrict__ out) {
    const int ng = d / 4;
    const long t = (long)blockIdx.x * WG + threadIdx.x;
    if (t >= n * ng) return;
    const long i = t / ng;
    const int g = (int)(t % ng);
    const float qn = __builtin_nanf("");
    f32x4 v = {0, 0, 0, 0};
    bool ok = true;
    for (int m = 0; m < M; m++) {
        const int code = codes[i * M + m];
        if (code >= ksub) {
            ok = false;
            break;
        }
        const f32x4 w = *reinterpret_cast<const f32x4*>(cb + ((size_t)m * ksub + code) * d + 4 * g);
        v = m == 0 ? w : v + w;
    }
    if (!ok) v = {qn, qn, qn, qn};
    *reinterpret_cast<f32x4*>(out + i * (long)d + 4 * g) = v;
}

__global__ void __launch_bounds__(WG)
rq_decode_scalar_kernel(const uint8_t* __restrict__ codes, long n, int d, int M, int ksub, const float* __restrict__ cb,
                        float* __restrict__ out) {
    const long t = (long)blockIdx.x * WG + threadIdx.x;
    if (t >= n * d) return;
    const long i = t / d;
    const int f = (int)(t % d);
    float v = 0.0f;
    bool ok = true;
    for (int m = 0; m < M; m++) {
        const int code = codes[i * M + m];
        if (code >= ksub) {
            ok = false;
            break;
        }
        const float w = cb[((size_t)m * ksub + code) * d + f];
        v = m == 0 ? w : v + w;
    }
    out[t] = ok ? v : __builtin_nanf("");
}

template <int NCH>
int launch_fused(at_ctx* ctx, const float* x, int64_t n, int M, int ksub, const float* cb, uint8_t* codes, float* dist,
                 float* resid, int32_t* bad, hipStream_t stream) {
    const int d = NCH * cs::DC;
    const int tps = (ksub + cs::tile_rows(NA) - 1) / cs::tile_rows(NA);
    const size_t tile_f = at_chunked_image_tile_floats(d, NA);
    float* img = static_cast<float*>(at_ws(ctx, WS_RQ_IMG, sizeof(float) * (size_t)M * tps * tile_f, stream));
    if (!img) return AT_E_NOMEM;
    if (ksub % cs::tile_rows(NA) == 0) {   // the [M * ksub][d] table is one image whose tiles m * tps .. are stage m
        const int rc = at_prep_chunked_image(ctx, cb, M * ksub, d, NA, img, stream);
        if (rc) return rc;
    } else {
        for (int m = 0; m < M; m++) {
            const int rc = at_prep_chunked_image(ctx, cb + (size_t)m * ksub * d, ksub, d, NA, img + (size_t)m * tps * tile_f,
                                                 stream);
            if (rc) return rc;
        }
    }
    const size_t lds = 2 * sizeof(float) * cs::buf_floats(NA);
    AT_RAISE_LDS(ctx, rq_fused_kernel<NCH>, lds);
    const int pack4 = M % 4 == 0 && (reinterpret_cast<uintptr_t>(codes) & 3u) == 0;
    AT_LAUNCH(rq_fused_kernel<NCH>, dim3((unsigned)((n + 127) / 128)), dim3(WG), lds, stream, x, (long)n, M, ksub, tps, img,
              cb, codes, dist, resid, bad, pack4);
    return AT_OK;
}

int encode_general(at_ctx* ctx, const float* x, int64_t n, int d, int M, int ksub, const float* cb, uint8_t* codes,
                   float* dist, float* resid, int32_t* bad, hipStream_t stream) {
    float* res = resid;
    if (!res) {
        res = static_cast<float*>(at_ws(ctx, WS_RQ_TMP, sizeof(float) * (size_t)n * d, stream));
        if (!res) return AT_E_NOMEM;
    }
    AT_LAUNCH(rq_general_kernel, dim3((unsigned)((n + RB - 1) / RB)), dim3(WG), 0, stream, x, (long)n, d, M, ksub, cb,
              n < 20 ? 1 : 0, res, codes, dist, bad);
    return AT_OK;
}

}  // namespace

extern "C" int at_rq_encode_f32(at_ctx* ctx, const float* x, int64_t n, int d, int M, int ksub, const float* codebooks,
                                uint8_t* codes, float* dist, float* residual, int32_t* bad, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_rq_encode_f32: ctx is null");
    AT_REQUIRE(n >= 0 && d > 0 && M > 0 && ksub >= 1 && ksub <= 256, "at_rq_encode_f32: bad sizes n=%lld d=%d M=%d ksub=%d",
               (long long)n, d, M, ksub);
    if (n == 0) return AT_OK;
    AT_REQUIRE(x && codebooks && codes, "at_rq_encode_f32: null pointer");
    AT_REQUIRE(n <= ((int64_t)1 << 38) / (M > d ? M : d), "at_rq_encode_f32: n=%lld too large", (long long)n);
    if (residual) {
        const char *xa = reinterpret_cast<const char*>(x), *ra = reinterpret_cast<const char*>(residual);
        const size_t bytes = sizeof(float) * (size_t)n * d;
        AT_REQUIRE(ra + bytes <= xa || xa + bytes <= ra, "at_rq_encode_f32: residual overlaps x");
    }
    AT_HIP(hipSetDevice(ctx->device));
    if (bad) AT_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), stream));

    int rc = at_guard_enter(&ctx->guard[AT_GUARD_RQ], stream);   // calls of one context share WS_RQ_IMG / WS_RQ_TMP
    if (rc) return rc;
    if ((d == 64 || d == 128) && n >= 20 && at_aligned16(x) && at_aligned16(codebooks) && at_aligned16(residual)) {
        if (d == 64) rc = launch_fused<1>(ctx, x, n, M, ksub, codebooks, codes, dist, residual, bad, stream);
        else rc = launch_fused<2>(ctx, x, n, M, ksub, codebooks, codes, dist, residual, bad, stream);
    } else {
        rc = encode_general(ctx, x, n, d, M, ksub, codebooks, codes, dist, residual, bad, stream);
    }
    if (rc) return rc;
    return at_guard_leave(&ctx->guard[AT_GUARD_RQ], stream);
}

extern "C" int at_rq_decode_f32(at_ctx* ctx, const uint8_t* codes, int64_t n, int d, int M, int ksub,
                                const float* codebooks, float* out, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_rq_decode_f32: ctx is null");
    AT_REQUIRE(n >= 0 && d > 0 && M > 0 && ksub >= 1 && ksub <= 256, "at_rq_decode_f32: bad sizes n=%lld d=%d M=%d ksub=%d",
               (long long)n, d, M, ksub);
    if (n == 0) return AT_OK;
    AT_REQUIRE(codes && codebooks && out, "at_rq_decode_f32: null pointer");
    AT_REQUIRE(n <= ((int64_t)1 << 38) / (M > d ? M : d), "at_rq_decode_f32: n=%lld too large", (long long)n);
    AT_HIP(hipSetDevice(ctx->device));
    if (d % 4 == 0 && at_aligned16(codebooks) && at_aligned16(out))
        AT_LAUNCH(rq_decode_vec_kernel, dim3((unsigned)((n * (d / 4) + WG - 1) / WG)), dim3(WG), 0, stream, codes, (long)n,
                  d, M, ksub, codebooks, out);
    else
        AT_LAUNCH(rq_decode_scalar_kernel, dim3((unsigned)((n * d + WG - 1) / WG)), dim3(WG), 0, stream, codes, (long)n, d,
                  M, ksub, codebooks, out);
    return AT_OK;
}
