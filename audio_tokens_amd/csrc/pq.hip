// pq.hip -- product quantiser on gfx950: at_pq_encode_f32 (ProductQuantizer.compute_codes) and at_pq_decode_f32.
//
// A frame of d features is cut into M sub-vectors of dsub = d / M features; sub-space m has a codebook of ksub rows.
// codes[i][m] is at_assign_f32's answer for sub-vector m of row i against codebook m, bit for bit (assign.hip, header):
//   ip, |x|^2, |c|^2 ascending fmaf chains over the dsub features from +0, dis = fma(-2, ip, xn + cn), the clamp
//   v < 0 ? 0 : v (a NaN stays a NaN), the lowest index among equal distances; calls with n < 20 rows use the direct
//   form sum (x-c)^2.  A sub-vector with no distance below +inf gets code 0, distance +inf, and raises *bad.
//
// Fused path (ksub == 256, dsub % 4 == 0, 16-byte aligned rows, n >= 20, image within the LDS budget): one launch.
// The codebooks are prepared once per call into an MFMA-operand image (WS_PQ_IMG): per sub-space [dsub/4][256][4]
// floats -- the four features of a group stored (f0, f2, f1, f3), so that the half-wave h of a lane reads its operands
// of the group's two v_mfma_f32_32x32x2_f32 (features 4g+h and 4g+2+h) with one 8-byte LDS load, and the 64 lanes of
// a wave read 512 contiguous bytes -- followed by the 256 |c|^2 chains.  Every workgroup copies the whole image
// (256 * (d + M) floats) into LDS once and then walks 32-row tiles, one per wave at a time, with a grid stride.  Per
// tile and sub-space a wave loads the sub-vectors of its 32 rows (both half-waves the same 16-byte pieces: every lane
// needs the whole |x|^2 chain), while the loads of the next sub-space are already in flight, and sweeps the 256
// centroids in two passes of four 32-centroid accumulators: dsub/2 MFMAs each, whose k order (group ascending, then
// the two k-pairs, then k = 0, 1 inside an instruction) is the ascending chain of the contract, exactly as in
// chunked_sweep.h.
// The accumulator puts the x row on the lane and 16 centroids in its registers; a lane meets its centroids in
// ascending index ((pass, accumulator, register) ascends for a fixed half-wave), so a running strict `<` minimum keeps
// the lowest index without comparing ids.  The two half-waves (same rows, disjoint centroids) merge once per
// sub-space, the lower index winning on equal distances.  Codes leave as one 32-bit store per four sub-spaces where M
// and the pointer allow, byte stores otherwise.
//
// General path (everything else): one thread per (row, sub-space) walks the codebook with the same scalar chains.
// Decode: a gather, 16 bytes per thread where dsub and the pointers allow, one float per thread otherwise.
#include "at_internal.h"
#include "chunked_sweep.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int KS = 256;                       // codebook rows of the fused path
constexpr int WG = 256;                       // prep, general and decode kernels
constexpr size_t LDS_BUDGET = 160 * 1024;     // the whole LDS of a CU: image + norms of d + M <= 160
constexpr size_t LDS_TWO_WGS = 80 * 1024;     // up to here two workgroups of 8 waves share a CU, above one of 16
using cs::clamp0;
using cs::NONE;

// one workgroup per sub-space, one thread per codebook row
__global__ void __launch_bounds__(KS)
pq_prep_kernel(const float* __restrict__ cb, int dsub, float* __restrict__ img) {
    const int m = blockIdx.x, r = threadIdx.x;
    const float* c = cb + ((size_t)m * KS + r) * dsub;
    float* im = img + (size_t)m * KS * (dsub + 1);
    float cn = 0.0f;
    for (int g = 0; g < dsub / 4; g++) {
        const float a0 = c[4 * g], a1 = c[4 * g + 1], a2 = c[4 * g + 2], a3 = c[4 * g + 3];
        cn = __builtin_fmaf(a0, a0, cn);
        cn = __builtin_fmaf(a1, a1, cn);
        cn = __builtin_fmaf(a2, a2, cn);
        cn = __builtin_fmaf(a3, a3, cn);
        const f32x4 v = {a0, a2, a1, a3};
        *reinterpret_cast<f32x4*>(im + ((size_t)g * KS + r) * 4) = v;
    }
    im[(size_t)KS * dsub + r] = cn;
}

// DSUB > 0: the sub-vector in registers, the next one prefetched; DSUB = 0: any dsub % 4 == 0, re-read per pass
template <int DSUB>
__global__ void __launch_bounds__(1024)
pq_fused_kernel(const float* __restrict__ X, long n, int d, int M, int dsub_rt, const float* __restrict__ img,
                int img_f4, uint8_t* __restrict__ codes, float* __restrict__ dist, int* __restrict__ bad, int pack4) {
    extern __shared__ __attribute__((aligned(16))) float smem[];   // 256 * (d + M) floats
    constexpr int NG = DSUB > 0 ? DSUB / 4 : 1;
    const int dsub = DSUB > 0 ? DSUB : dsub_rt;
    const int ng = dsub / 4;

    for (int i = threadIdx.x; i < img_f4; i += blockDim.x)
        reinterpret_cast<f32x4*>(smem)[i] = reinterpret_cast<const f32x4*>(img)[i];
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31;   // x row within the wave's 32 rows == accumulator column
    const int h = lane >> 5;   // which k of each MFMA k-pair this lane feeds
    const int wpb = blockDim.x >> 6;
    const long ntiles = (n + 31) / 32;
    const long tstride = (long)gridDim.x * wpb;
    long t = (long)blockIdx.x * wpb + wave;
    if (t >= ntiles) return;

    auto row_of = [&](long tt) {
        const long r = tt * 32 + j;
        return X + (r < n ? r : n - 1) * (long)d;
    };
    f32x4 raw[NG];
    const float* xrow = row_of(t);
    if constexpr (DSUB > 0) {
#pragma unroll
        for (int g = 0; g < NG; g++) raw[g] = *reinterpret_cast<const f32x4*>(xrow + 4 * g);
    }

    const cs::CodeSink sink{codes, dist, bad, pack4};
    for (; t < ntiles; t += tstride) {
        const long r = t * 32 + j;
        const bool store = h == 0 && r < n;
        const float* xnext = t + tstride < ntiles ? row_of(t + tstride) : xrow;
        unsigned pack = 0;
        for (int m = 0; m < M; m++) {
            const float* im = smem + (size_t)m * KS * (dsub + 1);
            const float* cnh = im + KS * dsub + 4 * h;   // the norms of this half-wave's centroids
            const float* xs = xrow + m * dsub;
            float xn = 0.0f;
            float xa[NG], xb[NG];
            if constexpr (DSUB > 0) {
#pragma unroll
                for (int g = 0; g < NG; g++) {
                    const f32x4 u = raw[g];
                    xn = __builtin_fmaf(u[0], u[0], xn);
                    xn = __builtin_fmaf(u[1], u[1], xn);
                    xn = __builtin_fmaf(u[2], u[2], xn);
                    xn = __builtin_fmaf(u[3], u[3], xn);
                    xa[g] = h ? u[1] : u[0];
                    xb[g] = h ? u[3] : u[2];
                }
                // the next sub-vector (of this tile, or the first of the wave's next tile) while this one is swept
                const float* nx = m + 1 < M ? xs + DSUB : xnext;
#pragma unroll
                for (int g = 0; g < NG; g++) raw[g] = *reinterpret_cast<const f32x4*>(nx + 4 * g);
            }

            float best = __builtin_inff();
            unsigned bcode = NONE;   // (pass * 4 + accumulator) * 16 + register
#pragma unroll 1
            for (int p = 0; p < 2; p++) {
                f32x16 acc[4];
#pragma unroll
                for (int a = 0; a < 4; a++) acc[a] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                const float* ap = im + (p * 128 + j) * 4 + 2 * h;
                if constexpr (DSUB > 0) {
#pragma unroll
                    for (int g = 0; g < NG; g++) {
                        f32x2 av[4];
#pragma unroll
                        for (int a = 0; a < 4; a++) av[a] = *reinterpret_cast<const f32x2*>(ap + (g * KS + a * 32) * 4);
#pragma unroll
                        for (int a = 0; a < 4; a++)
                            acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a][0], xa[g], acc[a], 0, 0, 0);
#pragma unroll
                        for (int a = 0; a < 4; a++)
                            acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a][1], xb[g], acc[a], 0, 0, 0);
                    }
                } else {
                    for (int g = 0; g < ng; g++) {
                        const f32x4 u = *reinterpret_cast<const f32x4*>(xs + 4 * g);
                        if (p == 0) {
                            xn = __builtin_fmaf(u[0], u[0], xn);
                            xn = __builtin_fmaf(u[1], u[1], xn);
                            xn = __builtin_fmaf(u[2], u[2], xn);
                            xn = __builtin_fmaf(u[3], u[3], xn);
                        }
                        const float xa0 = h ? u[1] : u[0], xb0 = h ? u[3] : u[2];
                        f32x2 av[4];
#pragma unroll
                        for (int a = 0; a < 4; a++) av[a] = *reinterpret_cast<const f32x2*>(ap + (g * KS + a * 32) * 4);
#pragma unroll
                        for (int a = 0; a < 4; a++)
                            acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a][0], xa0, acc[a], 0, 0, 0);
#pragma unroll
                        for (int a = 0; a < 4; a++)
                            acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a][1], xb0, acc[a], 0, 0, 0);
                    }
                }
                // accumulator register e holds centroid cs::acc_base(p * 4 + a, h) + cs::reg_offset(e): ascending in e
                // (the fences keep the norm loads of all four accumulators from being hoisted above the products)
#pragma unroll
                for (int a = 0; a < 4; a++) {
                    __builtin_amdgcn_sched_barrier(0);
                    const int ab = p * 4 + a;
                    cs::min16(acc[a], cnh + ab * 32, xn, (unsigned)(ab * 16), best, bcode);
                }
            }
            const unsigned win = cs::merged_index(best, bcode, h);
            sink.put(win, best, store, r * (long)M + m, m, pack);
        }
        xrow = xnext;
    }
}

// One thread per (row, sub-space): any dsub, any alignment, any ksub <= 256; direct: the call has n < 20 rows.
__global__ void __launch_bounds__(WG)
pq_general_kernel(const float* __restrict__ X, long n, int d, int M, int dsub, int ksub, const float* __restrict__ cb,
                  int direct, uint8_t* __restrict__ codes, float* __restrict__ dist, int* __restrict__ bad) {
    const long t = (long)blockIdx.x * WG + threadIdx.x;
    if (t >= n * M) return;
    const long i = t / M;
    const int m = (int)(t % M);
    const float* xi = X + i * (long)d + m * dsub;
    const float* cm = cb + (size_t)m * ksub * dsub;
    float xn = 0.0f;
    if (!direct)
        for (int f = 0; f < dsub; f++) xn = __builtin_fmaf(xi[f], xi[f], xn);
    float best = __builtin_inff();
    int bi = -1;
    for (int c = 0; c < ksub; c++) {
        const float* cc = cm + (size_t)c * dsub;
        float v;
        if (direct) {
            float acc = 0.0f;
            for (int f = 0; f < dsub; f++) {
                const float df = xi[f] - cc[f];
                acc = __builtin_fmaf(df, df, acc);
            }
            v = acc;
        } else {
            float cn = 0.0f, ip = 0.0f;
            for (int f = 0; f < dsub; f++) {
                cn = __builtin_fmaf(cc[f], cc[f], cn);
                ip = __builtin_fmaf(xi[f], cc[f], ip);
            }
            v = clamp0(__builtin_fmaf(-2.0f, ip, xn + cn));
        }
        if (v < best) {
            best = v;
            bi = c;
        }
    }
    codes[t] = (uint8_t)(bi < 0 ? 0 : bi);
    if (dist) dist[t] = best;
    if (bi < 0 && bad) *bad = 1;
}

// out[i][m * dsub + 4 * g ..] = codebook m, row codes[i][m], 16 bytes per thread; a code >= ksub decodes to NaN
__global__ void __launch_bounds__(WG)
pq_decode_vec_kernel(const uint8_t* __restrict__ codes, long n, int M, int dsub, int ksub, const float* __restrict__ cb,
                     float* __restrict__ out) {
    const int ng = dsub / 4;
    const long t = (long)blockIdx.x * WG + threadIdx.x;
    if (t >= n * M * ng) return;
    const int g = (int)(t % ng);
    const long im = t / ng;
    const int m = (int)(im % M);
    const int code = codes[im];
    const float qn = __builtin_nanf("");
    f32x4 v = {qn, qn, qn, qn};
    if (code < ksub) v = *reinterpret_cast<const f32x4*>(cb + ((size_t)m * ksub + code) * dsub + 4 * g);
    *reinterpret_cast<f32x4*>(out + im * dsub + 4 * g) = v;
}

__global__ void __launch_bounds__(WG)
pq_decode_scalar_kernel(const uint8_t* __restrict__ codes, long n, int d, int M, int dsub, int ksub,
                        const float* __restrict__ cb, float* __restrict__ out) {
    const long t = (long)blockIdx.x * WG + threadIdx.x;
    if (t >= n * d) return;
    const long i = t / d;
    const int f = (int)(t % d);
    const int m = f / dsub;
    const int code = codes[i * M + m];
    out[t] = code < ksub ? cb[((size_t)m * ksub + code) * dsub + (f - m * dsub)] : __builtin_nanf("");
}

template <int DSUB>
int launch_fused(at_ctx* ctx, const float* x, int64_t n, int d, int M, const float* img, size_t lds, uint8_t* codes,
                 float* dist, int32_t* bad, hipStream_t stream) {
    AT_RAISE_LDS(ctx, pq_fused_kernel<DSUB>, lds);
    const int wpb = lds <= LDS_TWO_WGS ? 8 : 16;
    const int64_t ntiles = (n + 31) / 32;
    int64_t grid = (ntiles + wpb - 1) / wpb;
    const int64_t resident = (int64_t)(ctx->n_cus > 0 ? ctx->n_cus : 256) * (wpb == 8 ? 2 : 1);
    if (grid > resident) grid = resident;
    const int pack4 = M % 4 == 0 && (reinterpret_cast<uintptr_t>(codes) & 3u) == 0;
    AT_LAUNCH(pq_fused_kernel<DSUB>, dim3((unsigned)grid), dim3(64 * wpb), lds, stream, x, (long)n, d, M, d / M, img,
              (int)(lds / 16), codes, dist, bad, pack4);
    return AT_OK;
}

}  // namespace

extern "C" int at_pq_encode_f32(at_ctx* ctx, const float* x, int64_t n, int d, int M, int ksub, const float* codebooks,
                                uint8_t* codes, float* dist, int32_t* bad, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_pq_encode_f32: ctx is null");
    AT_REQUIRE(n >= 0 && d > 0 && M > 0 && d % M == 0 && ksub >= 1 && ksub <= 256,
               "at_pq_encode_f32: bad sizes n=%lld d=%d M=%d ksub=%d", (long long)n, d, M, ksub);
    if (n == 0) return AT_OK;
    AT_REQUIRE(x && codebooks && codes, "at_pq_encode_f32: null pointer");
    AT_REQUIRE(n <= ((int64_t)1 << 38) / M, "at_pq_encode_f32: n=%lld too large", (long long)n);
    AT_HIP(hipSetDevice(ctx->device));
    if (bad) AT_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), stream));

    const int dsub = d / M;
    const size_t lds = sizeof(float) * KS * ((size_t)d + M);
    if (ksub == KS && dsub % 4 == 0 && at_aligned16(x) && n >= 20 && lds <= LDS_BUDGET) {
        int rc = at_guard_enter(&ctx->guard[AT_GUARD_PQ], stream);   // calls of one context share WS_PQ_IMG
        if (rc) return rc;
        float* img = static_cast<float*>(at_ws(ctx, WS_PQ_IMG, lds, stream));
        if (!img) return AT_E_NOMEM;
        AT_LAUNCH(pq_prep_kernel, dim3(M), dim3(KS), 0, stream, codebooks, dsub, img);
        if (dsub == 4) rc = launch_fused<4>(ctx, x, n, d, M, img, lds, codes, dist, bad, stream);
        else if (dsub == 8) rc = launch_fused<8>(ctx, x, n, d, M, img, lds, codes, dist, bad, stream);
        else if (dsub == 16) rc = launch_fused<16>(ctx, x, n, d, M, img, lds, codes, dist, bad, stream);
        else rc = launch_fused<0>(ctx, x, n, d, M, img, lds, codes, dist, bad, stream);
        if (rc) return rc;
        return at_guard_leave(&ctx->guard[AT_GUARD_PQ], stream);
    }
    AT_LAUNCH(pq_general_kernel, dim3((unsigned)((n * M + WG - 1) / WG)), dim3(WG), 0, stream, x, (long)n, d, M, dsub,
              ksub, codebooks, n < 20 ? 1 : 0, codes, dist, bad);
    return AT_OK;
}

extern "C" int at_pq_decode_f32(at_ctx* ctx, const uint8_t* codes, int64_t n, int d, int M, int ksub,
                                const float* codebooks, float* out, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_pq_decode_f32: ctx is null");
    AT_REQUIRE(n >= 0 && d > 0 && M > 0 && d % M == 0 && ksub >= 1 && ksub <= 256,
               "at_pq_decode_f32: bad sizes n=%lld d=%d M=%d ksub=%d", (long long)n, d, M, ksub);
    if (n == 0) return AT_OK;
    AT_REQUIRE(codes && codebooks && out, "at_pq_decode_f32: null pointer");
    AT_REQUIRE(n <= ((int64_t)1 << 38) / d, "at_pq_decode_f32: n=%lld too large", (long long)n);
    AT_HIP(hipSetDevice(ctx->device));
    const int dsub = d / M;
    if (dsub % 4 == 0 && at_aligned16(codebooks) && at_aligned16(out))
        AT_LAUNCH(pq_decode_vec_kernel, dim3((unsigned)((n * (d / 4) + WG - 1) / WG)), dim3(WG), 0, stream, codes,
                  (long)n, M, dsub, ksub, codebooks, out);
    else
        AT_LAUNCH(pq_decode_scalar_kernel, dim3((unsigned)((n * d + WG - 1) / WG)), dim3(WG), 0, stream, codes, (long)n,
                  d, M, dsub, ksub, codebooks, out);
    return AT_OK;
}
