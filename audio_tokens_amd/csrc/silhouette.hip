// silhouette.hip -- exact silhouette samples / score of a labelled sample, sklearn's float32 recipe in fp64.
//
// Reference call site: processors/cluster_creator.py:115-117 (ClusterCreator.evaluate_clustering):
// sklearn.metrics.silhouette_score(data, labels, sample_size=10000).  For float32 rows sklearn computes
// (metrics/cluster/_unsupervised.py silhouette_samples / _silhouette_reduce, metrics/pairwise.py
// _euclidean_distances_upcast / pairwise_distances_chunked):
//   d2(i,j)  = fl32(((-2 <x_i,x_j>) + |x_i|^2) + |x_j|^2)       dot and norms in fp64 of the fp32 rows
//   dist     = sqrt_rn(max(d2, 0)), 0 on the diagonal (the same sample, not duplicate rows)
//   S[i,c]   = fl32(sum over j in c of dist(i,j))                 fp64, j ascending (np.bincount)
//   a_i      = fl32(S[i,own] / (n_own - 1)),  b_i = min over c != own of fl32(S[i,c] / n_c)
//   s_i      = fl32(fl32(b - a) / max(a, b)), NaN -> 0
// Only the order of the fp64 dot products and norms differs from sklearn's BLAS; every fp32 rounding point is the same.
//
// Layout.  The rows are sorted by label (rocPRIM radix sort of the int64 labels, stable: the members of a cluster keep
// their ascending order, which is np.bincount's summation order), giving a permutation, the segment offsets and each
// position's segment.  A workgroup owns 256 queries (sorted positions; 64 per wave, one per lane in the walk) and walks
// every column j in sorted order in chunks of 32 rows:
//   1. the chunk's rows are staged in LDS as fp32 (once per workgroup, for its four waves; the next chunk is prefetched
//      into registers behind the matrix work), the queries once per call -- or once per 64-dimension slab and chunk
//      when d > 64;
//   2. each wave multiplies the 32 x 64 (j x query) tile with v_mfma_f64_16x16x4_f64 (j on the row axis, fp32 widened
//      to fp64 exactly) and turns it into distances in registers;
//   3. the distances go through LDS so that every lane holds one query and all lanes walk the same j sequence: the
//      segment boundaries are the same for the whole wave, and the per-cluster sums are plain fp64 adds in j order.
// No float atomics: each s_i is one lane's sequential sum, so two calls give the same bits.
#include <cmath>
#include <cstring>

#include "at_internal.h"
#include "at_sort.h"

namespace {

constexpr int WG = 256;
constexpr int QW = 256;        // queries per workgroup: 64 per wave
constexpr int JC = 32;         // columns per chunk: two 16-row MFMA tiles
constexpr int DS = 64;         // dimensions per slab (16 per lane group of the MFMA's k axis)
constexpr int LS = DS + 1;     // LDS row stride of staged rows (floats): lane (row c, group g) hits bank c + 16 g
constexpr int DSTR = 80;       // LDS row stride of a wave's distance tile: writes and reads conflict-free
constexpr int PF = JC * DS / WG;   // staged floats per thread and chunk

constexpr size_t LDS_Q = (size_t)QW * LS * 4;
constexpr size_t LDS_J = (size_t)JC * LS * 4;
constexpr size_t LDS_D = (size_t)(WG / 64) * JC * DSTR * 4;
constexpr size_t LDS_BYTES = LDS_Q + LDS_J + LDS_D + (size_t)JC * 8;

typedef double f64x4 __attribute__((ext_vector_type(4)));

__global__ void sil_iota_kernel(uint32_t* v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}

__global__ void sil_head_kernel(const int64_t* __restrict__ sk, int64_t n, uint32_t* __restrict__ head) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) head[p] = (p == 0 || sk[p] != sk[p - 1]) ? 1u : 0u;
}

// seg: inclusive scan of the heads (1-based segment of each position).  off[c] = first position of segment c,
// off[n_seg] = n; nrm[p] = |x_perm[p]|^2 in fp64.
__global__ void sil_segments_kernel(const float* __restrict__ x, int d, int64_t n, const uint32_t* __restrict__ perm,
                                    const uint32_t* __restrict__ head, const uint32_t* __restrict__ seg,
                                    uint32_t* __restrict__ off, double* __restrict__ nrm, int64_t* __restrict__ n_labels) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (head[p]) off[seg[p] - 1] = (uint32_t)p;
    if (p == n - 1) {
        off[seg[p]] = (uint32_t)n;
        *n_labels = (int64_t)seg[p];
    }
    const float* r = x + (size_t)perm[p] * d;
    double acc = 0.0;
    for (int k = 0; k < d; k++) {
        const double v = (double)r[k];
        acc += v * v;
    }
    nrm[p] = acc;
}

// one staged element e of (rows r0.., slab sl): row r0 + e / DS, dimension sl * DS + e % DS, zero outside
__device__ __forceinline__ float sil_elem(const float* __restrict__ x, int d, int64_t n, const uint32_t* __restrict__ perm,
                                          int64_t r0, int sl, int e) {
    const int64_t r = r0 + e / DS;
    const int k = sl * DS + e % DS;
    return (r < n && k < d) ? x[(size_t)perm[r] * d + k] : 0.0f;
}

__global__ __launch_bounds__(WG) void silhouette_kernel(const float* __restrict__ x, int d, int64_t n,
                                                        const uint32_t* __restrict__ perm, const uint32_t* __restrict__ seg,
                                                        const uint32_t* __restrict__ off, const double* __restrict__ nrm,
                                                        float* __restrict__ s) {
    extern __shared__ __align__(16) unsigned char sil_lds[];
    float* qs = reinterpret_cast<float*>(sil_lds);
    float* js = reinterpret_cast<float*>(sil_lds + LDS_Q);
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, g = l >> 4, c = l & 15;
    float* ds = reinterpret_cast<float*>(sil_lds + LDS_Q + LDS_J) + (size_t)w * JC * DSTR;
    double* jn = reinterpret_cast<double*>(sil_lds + LDS_Q + LDS_J + LDS_D);

    const int64_t q0 = (int64_t)blockIdx.x * QW + w * 64;   // this wave's first query
    const int nslab = (d + DS - 1) / DS;
    // the column norms of the MFMA tiles (query q0 + 16 t + c)
    double qn[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int64_t q = q0 + 16 * t + c;
        qn[t] = q < n ? nrm[q] : 0.0;
    }
    // walk state: lane l is query q0 + l
    const int64_t myq = q0 + l;
    const uint32_t own = myq < n ? seg[myq] - 1 : 0xffffffffu;
    double run = 0.0;            // sum over the current segment
    float a_sum = 0.0f;          // S[i, own]
    float b = INFINITY;
    uint32_t cur = 0;
    uint32_t cur_end = off[1];

    float pf[PF];
#pragma unroll
    for (int i = 0; i < PF; i++) pf[i] = sil_elem(x, d, n, perm, 0, 0, tid + i * WG);

    for (int64_t jb = 0; jb < n; jb += JC) {
        f64x4 acc[2][4];
#pragma unroll
        for (int u = 0; u < 2; u++)
#pragma unroll
            for (int t = 0; t < 4; t++) acc[u][t] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int sl = 0; sl < nslab; sl++) {
            __syncthreads();   // the previous slab's / chunk's readers are done with qs, js, ds
            if (jb == 0 || nslab > 1)
                for (int e = tid; e < QW * DS; e += WG)
                    qs[(e / DS) * LS + e % DS] = sil_elem(x, d, n, perm, (int64_t)blockIdx.x * QW, sl, e);
#pragma unroll
            for (int i = 0; i < PF; i++) {
                const int e = tid + i * WG;
                js[(e / DS) * LS + e % DS] = pf[i];
            }
            if (sl == 0 && tid < JC) jn[tid] = jb + tid < n ? nrm[jb + tid] : 0.0;
            __syncthreads();
            // prefetch the next (chunk, slab) step's rows behind the matrix work
            {
                int64_t nj = jb;
                int ns = sl + 1;
                if (ns == nslab) { ns = 0; nj += JC; }
#pragma unroll
                for (int i = 0; i < PF; i++) pf[i] = sil_elem(x, d, n, perm, nj, ns, tid + i * WG);
            }
            const float* ja = js + c * LS + 16 * g;
            const float* qb = qs + (w * 64 + c) * LS + 16 * g;
#pragma unroll 4
            for (int st = 0; st < 16; st++) {
                const double a0 = (double)ja[st], a1 = (double)ja[16 * LS + st];
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const double bq = (double)qb[16 * t * LS + st];
                    acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bq, acc[0][t], 0, 0, 0);
                    acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bq, acc[1][t], 0, 0, 0);
                }
            }
        }
        // distances: C/D of the f64 MFMA holds row (j) g + 4 r, column (query) c
#pragma unroll
        for (int u = 0; u < 2; u++)
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int jl = 16 * u + g + 4 * r;
                    const double d2 = (-2.0 * acc[u][t][r] + qn[t]) + jn[jl];
                    float f = (float)d2;
                    f = f > 0.0f ? f : 0.0f;
                    if (jb + jl == q0 + 16 * t + c) f = 0.0f;
                    // fp64 square root rounded to fp32: correctly rounded (53 >= 2 * 24 + 2), unlike v_sqrt_f32
                    ds[jl * DSTR + 16 * t + c] = (float)__builtin_sqrt((double)f);
                }
        __syncthreads();
        // the walk: every lane sees the same j, so a segment ends for the whole wave at once
        const int jend = (int)(n - jb < JC ? n - jb : JC);
        for (int jl = 0; jl < jend; jl++) {
            if ((uint32_t)(jb + jl) == cur_end) {
                const float S = (float)run;
                if (cur == own) a_sum = S;
                else b = fminf(b, (float)((double)S / (double)(cur_end - off[cur])));
                run = 0.0;
                cur++;
                cur_end = off[cur + 1];
            }
            run += (double)ds[jl * DSTR + l];
        }
    }
    if (myq >= n) return;
    {
        const float S = (float)run;   // the last segment
        if (cur == own) a_sum = S;
        else b = fminf(b, (float)((double)S / (double)(cur_end - off[cur])));
    }
    const double n_own = (double)(off[own + 1] - off[own]);
    const float a = (float)((double)a_sum / (n_own - 1.0));   // 0 / 0 = NaN for a singleton
    const float num = b - a;
    const float den = fmaxf(a, b);
    float sv = (float)((double)num / (double)den);             // fp64 quotient rounded once: correctly rounded
    if (sv != sv) sv = 0.0f;
    s[perm[myq]] = sv;
}

size_t sil_align(size_t b) { return (b + 255) & ~size_t(255); }

}  // namespace

extern "C" int at_silhouette_f32(at_ctx* ctx, const float* x, int d, const int64_t* labels, int64_t n, float* s,
                                 double* sum, int64_t* n_labels, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx && x && labels && s && sum && n_labels, "at_silhouette_f32: null pointer");
    AT_REQUIRE(d >= 1 && n >= 1 && n < ((int64_t)1 << 31), "at_silhouette_f32: bad sizes (d = %d, n = %lld)", d,
               (long long)n);
    AT_HIP(hipSetDevice(ctx->device));
    // scratch: sorted keys, iota, permutation, heads, segments, offsets, norms, rocPRIM temporary storage
    size_t sort_bytes = 0, scan_bytes = 0;
    AT_HIP(rocprim::radix_sort_pairs<at_radix_config>(nullptr, sort_bytes, labels, (int64_t*)nullptr, (const uint32_t*)nullptr,
                                                      (uint32_t*)nullptr, (size_t)n, 0, 64, stream));
    AT_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n,
                                   rocprim::plus<uint32_t>(), stream));
    const size_t un = (size_t)n;
    const size_t b_keys = sil_align(8 * un), b_u32 = sil_align(4 * un), b_off = sil_align(4 * (un + 1)),
                 b_nrm = sil_align(8 * un), b_tmp = sil_align(sort_bytes > scan_bytes ? sort_bytes : scan_bytes);
    const size_t total = b_keys + 4 * b_u32 + b_off + b_nrm + b_tmp;
    // The slot is the context's: a call on another stream than the previous one waits for it (at_sum_f32's rule).
    { const int rc = at_guard_enter(&ctx->guard[AT_GUARD_SIL], stream); if (rc) return rc; }
    unsigned char* w = static_cast<unsigned char*>(at_ws(ctx, WS_SILHOUETTE, total, stream));
    if (!w) return AT_E_NOMEM;
    int64_t* keys = reinterpret_cast<int64_t*>(w);
    uint32_t* iota = reinterpret_cast<uint32_t*>(w + b_keys);
    uint32_t* perm = reinterpret_cast<uint32_t*>(w + b_keys + b_u32);
    uint32_t* head = reinterpret_cast<uint32_t*>(w + b_keys + 2 * b_u32);
    uint32_t* seg = reinterpret_cast<uint32_t*>(w + b_keys + 3 * b_u32);
    uint32_t* off = reinterpret_cast<uint32_t*>(w + b_keys + 4 * b_u32);
    double* nrm = reinterpret_cast<double*>(w + b_keys + 4 * b_u32 + b_off);
    void* tmp = w + b_keys + 4 * b_u32 + b_off + b_nrm;

    const unsigned blocks = (unsigned)((n + WG - 1) / WG);
    AT_LAUNCH(sil_iota_kernel, dim3(blocks), dim3(WG), 0, stream, iota, n);
    AT_HIP(rocprim::radix_sort_pairs<at_radix_config>(tmp, sort_bytes, labels, keys, iota, perm, (size_t)n, 0, 64, stream));
    AT_LAUNCH(sil_head_kernel, dim3(blocks), dim3(WG), 0, stream, keys, n, head);
    AT_HIP(rocprim::inclusive_scan(tmp, scan_bytes, head, seg, (size_t)n, rocprim::plus<uint32_t>(), stream));
    AT_LAUNCH(sil_segments_kernel, dim3(blocks), dim3(WG), 0, stream, x, d, n, perm, head, seg, off, nrm, n_labels);
    AT_RAISE_LDS(ctx, silhouette_kernel, LDS_BYTES);
    AT_LAUNCH(silhouette_kernel, dim3((unsigned)((n + QW - 1) / QW)), dim3(WG), LDS_BYTES, stream, x, d, n, perm, seg, off,
              nrm, s);
    { const int rc = at_guard_leave(&ctx->guard[AT_GUARD_SIL], stream); if (rc) return rc; }
    return at_sum_f32(ctx, s, n, sum, stream);
}
