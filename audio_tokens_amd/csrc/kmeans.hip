// kmeans.hip -- the non-GEMM half of one Lloyd iteration on gfx950.
//
// Replaces, inside faiss.Kmeans.train (processors/cluster_creator.py:42-56 of danavery/audio-tokens):
//   subsample_training_set's row copy      -> at_gather_rows_f32
//   compute_centroids (accumulate)         -> at_centroid_accum_f32      (accum.hip)
//   compute_centroids (1/count scaling)    -> at_centroid_finalize_f32   (+ data-parallel combine)
//   the objective  sum_i dis[i]            -> at_sum_f32
//   the isfinite() scan of the input       -> at_any_nonfinite_f32
//
// All of these are HBM-bound passes over [n][d] fp32 rows (4d+8 B per point per iteration).
//
// compute_centroids' accumulation (member lists in ascending point index, one wavefront per list) is in accum.hip.
#include <cstdlib>
#include <cstring>

#include "at_internal.h"

namespace {

constexpr int WG = 256;

__global__ void __launch_bounds__(WG) gather_rows_kernel(const float* __restrict__ x, int d4,
                                                         const int32_t* __restrict__ idx, long m,
                                                         float* __restrict__ out) {
    // one 16-byte chunk per thread; consecutive threads walk one row, then the next
    const long e = (long)blockIdx.x * WG + threadIdx.x;
    if (e >= m * d4) return;
    const long r = e / d4;
    const int c = (int)(e - r * d4);
    const float4* src = reinterpret_cast<const float4*>(x) + (long)idx[r] * d4 + c;
    reinterpret_cast<float4*>(out)[e] = *src;
}

__global__ void __launch_bounds__(WG) gather_rows_scalar_kernel(const float* __restrict__ x, int d,
                                                                const int32_t* __restrict__ idx,
                                                                long m, float* __restrict__ out) {
    const long e = (long)blockIdx.x * WG + threadIdx.x;
    if (e >= m * d) return;
    const long r = e / d;
    const int c = (int)(e - r * d);
    out[e] = x[(long)idx[r] * d + c];
}

__global__ void __launch_bounds__(WG) centroid_finalize_kernel(const float* __restrict__ sums_parts,
                                                               long sums_stride,
                                                               const float* __restrict__ counts_parts,
                                                               long counts_stride, int n_parts, int k,
                                                               int d,
                                                               float* __restrict__ cent,
                                                               float* __restrict__ hassign) {
    const long e = (long)blockIdx.x * WG + threadIdx.x;
    if (e >= (long)k * d) return;
    const int c = (int)(e / d);
    float cnt = 0.0f, tot = 0.0f;
    for (int p = 0; p < n_parts; p++) {
        cnt += counts_parts[p * counts_stride + c];
        tot += sums_parts[p * sums_stride + e];
    }
    float out = 0.0f;
    if (cnt != 0.0f) {
        const float inv = 1.0f / cnt;  // IEEE division, then one multiply: faiss' "norm = 1 / hassign"
        out = tot * inv;
    }
    cent[e] = out;
    if (e == (long)c * d) hassign[c] = cnt;
}

// out[i] = ((parts[0][i] + parts[1][i]) + parts[2][i]) + ...: the rank-ordered sum of the scatter form of the exchange
__global__ void __launch_bounds__(WG) sum_parts_kernel(const float* __restrict__ parts, long stride, int n_parts, long m,
                                                       float* __restrict__ out) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    if (i >= m) return;
    float tot = 0.0f;
    for (int p = 0; p < n_parts; p++) tot += parts[p * stride + i];
    out[i] = tot;
}

// ---- fixed-tree reductions ---------------------------------------------------------------------
constexpr int RED_BLOCKS = 1024;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// One launch: every workgroup leaves its partial sum, the last one to arrive (a counter that it also puts back to
// zero) adds the partials up in index order.  The result is a fixed function of (v, n): the grid is a function of n
// alone and every tree below is fixed, so repeated calls and all ranks agree bit for bit.  (It is NOT the partition
// round 1's two-kernel form used: the grid was capped at 256 / 1024 workgroups in round 2.  The objective it feeds is
// the one statistic the contract holds to a tolerance)
__global__ void __launch_bounds__(WG) sum_kernel(const float* __restrict__ v, long n, double* __restrict__ partial,
                                                 unsigned* __restrict__ ticket, double* __restrict__ out) {
    __shared__ double sh[WG / 64];
    __shared__ bool last;
    double acc = 0.0;
    for (long i = (long)blockIdx.x * WG + threadIdx.x; i < n; i += (long)gridDim.x * WG) acc += (double)v[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(&partial[blockIdx.x], (sh[0] + sh[1]) + (sh[2] + sh[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;          // (uniform over the workgroup)
    __threadfence();
    const int m = (int)gridDim.x;
    acc = 0.0;
    for (int i = threadIdx.x; i < m; i += WG) acc += __hip_atomic_load(&partial[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    acc = wave_sum(acc);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        *out = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        *ticket = 0u;
    }
}

__global__ void __launch_bounds__(WG) nonfinite_kernel(const float* __restrict__ v, long n,
                                                       int32_t* __restrict__ flag) {
    bool bad = false;
    for (long i = (long)blockIdx.x * WG + threadIdx.x; i < n; i += (long)gridDim.x * WG) {
        const uint32_t bits = __float_as_uint(v[i]);
        bad |= (bits & 0x7f800000u) == 0x7f800000u;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// Token histogram (spec_tokenizer.py:129-147 counts tokens with a Python
// Counter over tokens.tolist()).  Workgroup-private counts in LDS when the vocabulary fits, one
// global atomic per non-empty bin and workgroup afterwards.
constexpr int HIST_LDS_BINS = 16384;

__global__ void __launch_bounds__(WG) histogram_kernel(const long* __restrict__ ids, long n, int k,
                                                       unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned int bins[];
    const bool local = k <= HIST_LDS_BINS;
    if (local) {
        for (int b = threadIdx.x; b < k; b += WG) bins[b] = 0u;
        __syncthreads();
    }
    for (long i = (long)blockIdx.x * WG + threadIdx.x; i < n; i += (long)gridDim.x * WG) {
        const long t = ids[i];
        if (t < 0 || t >= k) continue;  // rows without a token (-1) are not counted
        if (local) atomicAdd(&bins[t], 1u);
        else atomicAdd(&counts[t], 1ull);
    }
    if (local) {
        __syncthreads();
        for (int b = threadIdx.x; b < k; b += WG)
            if (bins[b]) atomicAdd(&counts[b], (unsigned long long)bins[b]);
    }
}

}  // namespace

extern "C" {

int at_gather_rows_f32(at_ctx* ctx, const float* x, int d, const int32_t* idx, int64_t m, float* out,
                       void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx, "at_gather_rows_f32: ctx is null");
    AT_REQUIRE(m >= 0 && d > 0, "at_gather_rows_f32: bad sizes");
    if (m == 0) return AT_OK;
    AT_REQUIRE(x && idx && out, "at_gather_rows_f32: null pointer");
    AT_HIP(hipSetDevice(ctx->device));
    if (d % 4 == 0 && at_aligned16(x) && at_aligned16(out)) {
        const long total = m * (d / 4);
        AT_LAUNCH(gather_rows_kernel, dim3((unsigned)((total + WG - 1) / WG)), dim3(WG), 0,
                           stream, x, d / 4, idx, (long)m, out);
    } else {
        const long total = m * d;
        AT_LAUNCH(gather_rows_scalar_kernel, dim3((unsigned)((total + WG - 1) / WG)), dim3(WG),
                           0, stream, x, d, idx, (long)m, out);
    }
    return AT_OK;
}

int at_centroid_finalize_f32(at_ctx* ctx, const float* sums_parts, int64_t sums_part_stride,
                             const float* counts_parts, int64_t counts_part_stride, int n_parts,
                             int k, int d, float* centroids, float* hassign, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx, "at_centroid_finalize_f32: ctx is null");
    AT_REQUIRE(n_parts >= 1 && k > 0 && d > 0, "at_centroid_finalize_f32: bad sizes");
    AT_REQUIRE(sums_parts && counts_parts && centroids && hassign, "at_centroid_finalize_f32: null pointer");
    AT_HIP(hipSetDevice(ctx->device));
    const long total = (long)k * d;
    AT_LAUNCH(centroid_finalize_kernel, dim3((unsigned)((total + WG - 1) / WG)), dim3(WG), 0,
                       stream, sums_parts, (long)sums_part_stride, counts_parts,
                       (long)counts_part_stride, n_parts, k, d, centroids, hassign);
    return AT_OK;
}

int at_sum_parts_f32(at_ctx* ctx, const float* parts, int64_t part_stride, int n_parts, int64_t m, float* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx && n_parts >= 1 && m >= 0 && (m == 0 || (parts && out)), "at_sum_parts_f32: bad arguments");
    if (m == 0) return AT_OK;
    AT_HIP(hipSetDevice(ctx->device));
    AT_LAUNCH(sum_parts_kernel, dim3((unsigned)((m + WG - 1) / WG)), dim3(WG), 0, stream, parts, (long)part_stride,
                       n_parts, (long)m, out);
    return AT_OK;
}

int at_sum_f32(at_ctx* ctx, const float* v, int64_t n, double* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx && out && n >= 0 && (n == 0 || v), "at_sum_f32: bad arguments");
    AT_HIP(hipSetDevice(ctx->device));
    double* partial = static_cast<double*>(at_ws(ctx, WS_REDUCE, RED_BLOCKS * sizeof(double), stream));
    if (!partial) return AT_E_NOMEM;
    // one workgroup per CU at most: every workgroup ends with an atomic on the one arrival counter, and a thousand of
    // those in a row cost more (15 us) than the sum itself
    int blocks = (int)((n + 4 * WG - 1) / (4 * WG));
    const int cap = n <= ((int64_t)1 << 22) ? 256 : RED_BLOCKS;   // (long vectors want the bandwidth of more workgroups)
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    const bool fresh = ctx->ws[WS_SUM_TICKET] == nullptr;
    unsigned* ticket = static_cast<unsigned*>(at_ws(ctx, WS_SUM_TICKET, 16, stream));
    if (!ticket) return AT_E_NOMEM;
    if (fresh) AT_HIP(hipMemsetAsync(ticket, 0, 16, stream));
    // The partial buffer and the arrival counter are the context's: two calls on different streams must not overlap
    // (the wrong "last workgroup", a mixed sum, a counter that is never put back).  A call on another stream than the
    // previous one waits for it.
    { const int rc = at_guard_enter(&ctx->guard[AT_GUARD_SUM], stream); if (rc) return rc; }
    AT_LAUNCH(sum_kernel, dim3(blocks), dim3(WG), 0, stream, v, (long)n, partial, ticket, out);
    return at_guard_leave(&ctx->guard[AT_GUARD_SUM], stream);
}

int at_any_nonfinite_f32(at_ctx* ctx, const float* v, int64_t n, int32_t* flag, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx && flag && n >= 0 && (n == 0 || v), "at_any_nonfinite_f32: bad arguments");
    AT_HIP(hipSetDevice(ctx->device));
    AT_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), stream));
    if (n == 0) return AT_OK;
    int blocks = (int)((n + WG - 1) / WG);
    if (blocks > 2048) blocks = 2048;
    AT_LAUNCH(nonfinite_kernel, dim3(blocks), dim3(WG), 0, stream, v, (long)n, flag);
    return AT_OK;
}

int at_token_histogram_i64(at_ctx* ctx, const int64_t* ids, int64_t n, int k, int64_t* counts, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx && counts && k > 0 && n >= 0 && (n == 0 || ids), "at_token_histogram_i64: bad arguments");
    AT_HIP(hipSetDevice(ctx->device));
    AT_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)k, stream));
    if (n == 0) return AT_OK;
    int blocks = (int)((n + WG * 16 - 1) / (WG * 16));
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    const size_t lds = k <= HIST_LDS_BINS ? sizeof(unsigned int) * (size_t)k : 0;
    AT_RAISE_LDS(ctx, histogram_kernel, lds);
    AT_LAUNCH(histogram_kernel, dim3(blocks), dim3(WG), lds, stream, reinterpret_cast<const long*>(ids), (long)n, k,
                       reinterpret_cast<unsigned long long*>(counts));
    return AT_OK;
}

}  // extern "C"
