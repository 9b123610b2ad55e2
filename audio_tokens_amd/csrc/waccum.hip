// waccum.hip -- compute_centroids (accumulate) with per-row weights on gfx950: at_centroid_accum_weighted_f32.
//
// The contract: for cluster c with members i0 < i1 < ... (ascending row),
//     sums[c][f] = the chain s <- fmaf(x[i][f], w[i], s) from +0, one rounding per member,
//     wsums[c]   = the chain s <- s + w[i] from +0, in the same order.
// Every fused multiply-add is written out as __builtin_fmaf (the library is built with -ffp-contract=off); a product
// rounded before it is added would be another number.  No float atomics: the bits do not depend on the launch.
//
// Member lists: a stable radix sort of (id, row) pairs (at_sort.h) and the segment starts by binary search, as in the
// sort strategy of accum.hip -- in workspace slots of ITS OWN (WS_WACC_*), so a weighted call never touches what
// at_centroid_accum_f32 or its side stream are using.  Calls of one context share those slots: a call on another
// stream than the previous one waits for it (AT_GUARD_WACC).  Everything is queued on the caller's stream, in
// sequence: sort, offsets, short lists, long lists.  (accum.hip's predicted early lists, bucket strategy and side
// stream are left out on purpose; make_keys / the binary search are repeated here because accum.hip keeps its own in
// an unnamed namespace and stays as it is.)
#include <cstdlib>
#include <cstring>

#include "at_internal.h"
#include "at_sort.h"

namespace {

constexpr int WG = 256;

// Lists of up to WLONG_LIST members are one wave's walk (wcentroid_accum_kernel); longer ones are cut across features
// (wcentroid_accum_long_kernel), WLONG_CHUNK members per ring buffer.  The short kernel fetches WSHORT_RB / _RB_WIDE
// rows per register set (lanes with 1 or 2 / with 4 features).  at_waccum_limits hands all four to the tests.
constexpr uint32_t WLONG_LIST = 1024;
constexpr int WLONG_CHUNK = 1536;
constexpr int WSHORT_RB = 16, WSHORT_RB_WIDE = 8;

__global__ void __launch_bounds__(WG) wmake_keys_kernel(const long* __restrict__ ids, long n, int k,
                                                        uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const long c = ids[i];
    // an id outside [0, k) is parked in a trailing bucket that no centroid reads
    keys[i] = (c >= 0 && c < k) ? (uint32_t)c : (uint32_t)k;
    vals[i] = (uint32_t)i;
}

__device__ __forceinline__ uint32_t first_not_below(const uint32_t* __restrict__ keys, long n, uint32_t c) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (keys[mid] < c) lo = mid + 1; else hi = mid;
    }
    return (uint32_t)lo;
}

// offsets[c] = first position p of the sorted keys with keys[p] >= c, for c in [0, k]; the clusters with more than
// long_list members go into longs[1 ..] (any order: it decides which workgroup sums a list, not a bit of the sum),
// longs[0] = how many (zero before the launch).
__global__ void __launch_bounds__(WG) wsegment_offsets_kernel(const uint32_t* __restrict__ keys, long n, int k,
                                                              uint32_t long_list, uint32_t* __restrict__ offsets,
                                                              int* __restrict__ longs) {
    const int c = blockIdx.x * WG + threadIdx.x;
    if (c > k) return;
    const uint32_t beg = first_not_below(keys, n, (uint32_t)c);
    offsets[c] = beg;
    if (c == k || !longs) return;
    const uint32_t end = first_not_below(keys, n, (uint32_t)c + 1u);
    if (end - beg > long_list) longs[1 + atomicAdd(&longs[0], 1)] = c;
}

// One wavefront per (cluster, 64*VEC-feature slab).  Lane owns VEC consecutive features.  Of each block of 64 members
// lane l holds member l's row index and its weight; both are broadcast with readlane when their turn comes, so the
// weight of a row costs the wave one 4-byte load per 64 members and lane.  The weight chain ws is the same value in
// every lane (a vector add of a uniform operand); lane 0 of the cluster's first slab stores it.
template <int VEC>
__global__ void __launch_bounds__(WG) wcentroid_accum_kernel(const float* __restrict__ x, const float* __restrict__ w, int d,
                                                             const uint32_t* __restrict__ order,
                                                             const uint32_t* __restrict__ offsets, int k, int slabs,
                                                             uint32_t long_list, float* __restrict__ sums,
                                                             float* __restrict__ wsums) {
    const int lane = threadIdx.x & 63;
    const long wv = (long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (wv >= (long)k * slabs) return;
    const int c = (int)(wv / slabs);
    const int slab = (int)(wv - (long)c * slabs);
    const int f0 = (slab * 64 + lane) * VEC;
    const bool live = f0 < d;  // d is a multiple of VEC
    const uint32_t beg = offsets[c], end = offsets[c + 1];
    if (end - beg > long_list) return;  // left to wcentroid_accum_long_kernel

    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; v++) acc[v] = 0.0f;
    float ws = 0.0f;

    // Rows are fetched RB at a time into one of two register sets: the loads of batch i+1 are in flight while batch i
    // is multiplied and added, in member order (one dependent chain per feature), and the indices and weights of the
    // next 64 members are fetched while this block of 64 is summed.
    constexpr int RB = VEC == 4 ? WSHORT_RB_WIDE : WSHORT_RB;
    auto fetch = [&](uint32_t mine, uint32_t m, uint32_t cnt, float (&t)[RB][VEC]) {
#pragma unroll
        for (int u = 0; u < RB; u++) {
            const uint32_t src = __builtin_amdgcn_readlane(mine, (m + u) & 63);
            const bool ok = (m + u < cnt) && live;
            if constexpr (VEC == 4) {
                float4 q = ok ? *reinterpret_cast<const float4*>(x + (size_t)src * d + f0) : make_float4(0, 0, 0, 0);
                t[u][0] = q.x; t[u][1] = q.y; t[u][2] = q.z; t[u][3] = q.w;
            } else if constexpr (VEC == 2) {
                float2 q = ok ? *reinterpret_cast<const float2*>(x + (size_t)src * d + f0) : make_float2(0, 0);
                t[u][0] = q.x; t[u][1] = q.y;
            } else {
                t[u][0] = ok ? x[(size_t)src * d + f0] : 0.0f;
            }
        }
    };
    auto add = [&](uint32_t wmine, uint32_t m, uint32_t cnt, const float (&t)[RB][VEC]) {
#pragma unroll
        for (int u = 0; u < RB; u++) {
            if (m + u < cnt) {  // wave-uniform: the tail adds nothing at all
                const float wt = __uint_as_float(__builtin_amdgcn_readlane(wmine, (m + u) & 63));
#pragma unroll
                for (int v = 0; v < VEC; v++) acc[v] = __builtin_fmaf(t[u][v], wt, acc[v]);
                ws = ws + wt;
            }
        }
    };
    auto members = [&](uint32_t base, uint32_t* mine, uint32_t* wmine) {   // (base < end)
        const bool have = lane < min(64u, end - base);
        *mine = have ? order[base + lane] : 0u;
        *wmine = have ? __float_as_uint(w[*mine]) : 0u;
    };
    uint32_t mine_next = 0, wmine_next = 0;
    if (beg < end) members(beg, &mine_next, &wmine_next);
    for (uint32_t base = beg; base < end; base += 64) {
        const uint32_t cnt = min(64u, end - base);
        const uint32_t mine = mine_next, wmine = wmine_next;
        if (base + 64 < end) members(base + 64, &mine_next, &wmine_next);
        float tA[RB][VEC], tB[RB][VEC];
        fetch(mine, 0, cnt, tA);
        for (uint32_t m = 0; m < cnt; m += 2 * RB) {
            if (m + RB < cnt) fetch(mine, m + RB, cnt, tB);
            add(wmine, m, cnt, tA);
            if (m + RB < cnt) {
                if (m + 2 * RB < cnt) fetch(mine, m + 2 * RB, cnt, tA);
                add(wmine, m + RB, cnt, tB);
            }
        }
    }
    if (live) {
#pragma unroll
        for (int v = 0; v < VEC; v++) sums[(size_t)c * d + f0 + v] = acc[v];
    }
    if (slab == 0 && lane == 0) wsums[c] = ws;
}

// Long member lists: L dependent fused multiply-adds per feature, which one wave walking the list alone would pace the
// whole launch with.  As in accum.hip such a cluster is cut ACROSS FEATURES: one workgroup per (long cluster,
// 4-feature slice).  Waves 1-3 stream that 16-byte slice of every member row and the member's weight, in member order,
// into a double-buffered feature-major LDS ring (all index loads, then all row and weight loads, then the LDS writes);
// five lanes of wave 0 run the chains from 16-byte LDS reads: lanes 0-3 acc <- fmaf(x, w, acc) for their feature (the
// product is never rounded: the weights ride in a ring row of their own and meet the rows in the adder), lane 4 the
// weight chain, written as fmaf(w, 1, acc) so that the five lanes execute one instruction stream -- w * 1 is exact,
// hence the single rounding of acc + w.
constexpr int WLONG_LOADERS = WG - 64;
constexpr int WLONG_PER_THREAD = (WLONG_CHUNK + WLONG_LOADERS - 1) / WLONG_LOADERS;
constexpr int WLONG_GRID = 64;   // workgroups per feature slice; they stride over the long clusters
static_assert(WLONG_CHUNK % 64 == 0, "the adder reads the ring in batches of 64 members");
static_assert(2 * 5 * WLONG_CHUNK * sizeof(float) <= 64 * 1024, "the ring is static LDS");

__global__ void __launch_bounds__(WG) wcentroid_accum_long_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                  int d, const uint32_t* __restrict__ order,
                                                                  const uint32_t* __restrict__ offsets,
                                                                  uint32_t long_list, float* __restrict__ sums,
                                                                  float* __restrict__ wsums, int k,
                                                                  const int* __restrict__ longs) {
    // ring[buffer][row][member]: rows 0-3 the slice's features, row 4 the weights
    __shared__ __attribute__((aligned(16))) float ring[2][5][WLONG_CHUNK];
    const int n_slot = min(longs[0], k);
    const int piece = blockIdx.y;  // features 4*piece .. 4*piece+3
    const int tid = threadIdx.x;
    const bool adder = tid < 64;
    const float4* rows = reinterpret_cast<const float4*>(x) + piece;
    const int d4 = d >> 2;
    for (int slot = blockIdx.x; slot < n_slot; slot += gridDim.x) {
        const int c = longs[1 + slot];
        if (c < 0 || c >= k) continue;
        const uint32_t beg = offsets[c], len = offsets[c + 1] - beg;
        if (len <= long_list) continue;  // uniform for the workgroup
        const uint32_t nchunks = (len + WLONG_CHUNK - 1) / WLONG_CHUNK;

        auto stage = [&](uint32_t ch) {  // loaders only
            const uint32_t m0 = ch * WLONG_CHUNK;
            const uint32_t cnt = min((uint32_t)WLONG_CHUNK, len - m0);
            const uint32_t t = tid - 64;
            uint32_t src[WLONG_PER_THREAD];
            float4 v[WLONG_PER_THREAD];
            float wt[WLONG_PER_THREAD];
#pragma unroll
            for (int u = 0; u < WLONG_PER_THREAD; u++) {
                const uint32_t e = t + u * WLONG_LOADERS;
                src[u] = e < cnt ? order[beg + m0 + e] : 0u;
            }
#pragma unroll
            for (int u = 0; u < WLONG_PER_THREAD; u++) {
                const uint32_t e = t + u * WLONG_LOADERS;
                v[u] = e < cnt ? rows[(size_t)src[u] * d4] : make_float4(0, 0, 0, 0);
                wt[u] = e < cnt ? w[src[u]] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < WLONG_PER_THREAD; u++) {
                const uint32_t e = t + u * WLONG_LOADERS;
                if (e < cnt) {
                    ring[ch & 1][0][e] = v[u].x;
                    ring[ch & 1][1][e] = v[u].y;
                    ring[ch & 1][2][e] = v[u].z;
                    ring[ch & 1][3][e] = v[u].w;
                    ring[ch & 1][4][e] = wt[u];
                }
            }
        };

        float acc = 0.0f;
        if (!adder) stage(0);
        __syncthreads();
        for (uint32_t ch = 0; ch < nchunks; ch++) {
            if (!adder) {
                if (ch + 1 < nchunks) stage(ch + 1);
            } else if (tid < 5) {
                const float* src = ring[ch & 1][tid];          // lane 4: the weights themselves
                const float* wr = ring[ch & 1][4];
                const bool plain = tid == 4;                   // ... times one
                const uint32_t cnt = min((uint32_t)WLONG_CHUNK, len - ch * WLONG_CHUNK);
                uint32_t m = 0;
                for (; m + 64 <= cnt; m += 64) {   // the LDS latency is paid once per 64 members
                    float4 t[16], q[16];
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        t[u] = *reinterpret_cast<const float4*>(src + m + 4 * u);
                        q[u] = *reinterpret_cast<const float4*>(wr + m + 4 * u);
                    }
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        acc = __builtin_fmaf(t[u].x, plain ? 1.0f : q[u].x, acc);
                        acc = __builtin_fmaf(t[u].y, plain ? 1.0f : q[u].y, acc);
                        acc = __builtin_fmaf(t[u].z, plain ? 1.0f : q[u].z, acc);
                        acc = __builtin_fmaf(t[u].w, plain ? 1.0f : q[u].w, acc);
                    }
                }
                for (; m + 16 <= cnt; m += 16) {
                    float4 t[4], q[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        t[u] = *reinterpret_cast<const float4*>(src + m + 4 * u);
                        q[u] = *reinterpret_cast<const float4*>(wr + m + 4 * u);
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        acc = __builtin_fmaf(t[u].x, plain ? 1.0f : q[u].x, acc);
                        acc = __builtin_fmaf(t[u].y, plain ? 1.0f : q[u].y, acc);
                        acc = __builtin_fmaf(t[u].z, plain ? 1.0f : q[u].z, acc);
                        acc = __builtin_fmaf(t[u].w, plain ? 1.0f : q[u].w, acc);
                    }
                }
                for (; m < cnt; m++) acc = __builtin_fmaf(src[m], plain ? 1.0f : wr[m], acc);
            }
            __syncthreads();
        }
        if (tid < 4) sums[(size_t)c * d + 4 * piece + tid] = acc;
        if (tid == 4 && piece == 0) wsums[c] = acc;
        __syncthreads();   // (the ring is reused by the next list)
    }
}

// ---- host driver ------------------------------------------------------------------------------------------------
#define AT_TRY(expr) do { const int rc_ = (expr); if (rc_ != AT_OK) return rc_; } while (0)

int waccum_queue(at_ctx* ctx, const float* x, const float* w, long n, int d, const long* ids, int k, float* sums, float* wsums,
                 uint32_t* order_out, uint32_t* sorted_ids_out, hipStream_t stream) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    uint32_t* keys_a = static_cast<uint32_t*>(at_ws(ctx, WS_WACC_KEYS_A, nn * 4, stream));
    uint32_t* keys_b = static_cast<uint32_t*>(at_ws(ctx, WS_WACC_KEYS_B, nn * 4, stream));
    uint32_t* vals_a = static_cast<uint32_t*>(at_ws(ctx, WS_WACC_VALS_A, nn * 4, stream));
    uint32_t* vals_b = static_cast<uint32_t*>(at_ws(ctx, WS_WACC_VALS_B, nn * 4, stream));
    // WS_WACC_SEG, in words: offsets[k + 2] | longs[k + 1]
    uint32_t* offsets = static_cast<uint32_t*>(at_ws(ctx, WS_WACC_SEG, ((size_t)2 * k + 3) * 4, stream));
    if (!keys_a || !keys_b || !vals_a || !vals_b || !offsets) return AT_E_NOMEM;
    int* longs = reinterpret_cast<int*>(offsets + k + 2);

    // The feature-sliced kernel reads 16-byte slices of the rows: without them every list is a short one, walked
    // by the scalar-lane form of the short kernel (same order, same bits).
    const bool al = at_aligned16(x), long_ok = d % 4 == 0 && al;
    const uint32_t long_list = long_ok ? WLONG_LIST : UINT32_MAX;
    const long max_long = long_ok ? n / ((long)WLONG_LIST + 1) : 0;   // as many lists can be that long
    const int vec = d % 4 == 0 && d >= 256 && al ? 4 : d % 2 == 0 && d >= 128 && al ? 2 : 1;
    const int slabs = (d + 64 * vec - 1) / (64 * vec);

    const uint32_t *order = vals_a, *sorted_keys = keys_a;
    if (n > 0) {
        AT_LAUNCH(wmake_keys_kernel, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, stream, ids, n, k, keys_a, vals_a);
        unsigned bits = 1;
        while ((1u << bits) <= (unsigned)k) bits++;  // keys take values 0..k
        rocprim::double_buffer<uint32_t> kb(keys_a, keys_b);
        rocprim::double_buffer<uint32_t> vb(vals_a, vals_b);
        AT_TRY(at_sort_pairs(ctx, WS_WACC_TMP, kb, vb, (size_t)n, 0, bits, stream));
        order = vb.current(), sorted_keys = kb.current();
    }
    if (max_long > 0) AT_HIP(hipMemsetAsync(longs, 0, 4, stream));
    AT_LAUNCH(wsegment_offsets_kernel, dim3((k + 1 + WG - 1) / WG), dim3(WG), 0, stream, sorted_keys, n, k, long_list, offsets,
              max_long > 0 ? longs : nullptr);
    auto* short_kernel = vec == 4 ? wcentroid_accum_kernel<4> : vec == 2 ? wcentroid_accum_kernel<2> : wcentroid_accum_kernel<1>;
    AT_LAUNCH(short_kernel, dim3((unsigned)(((long)k * slabs + WG / 64 - 1) / (WG / 64))), dim3(WG), 0, stream, x, w, d, order,
              offsets, k, slabs, long_list, sums, wsums);
    if (max_long > 0)
        AT_LAUNCH(wcentroid_accum_long_kernel, dim3((unsigned)(max_long < WLONG_GRID ? max_long : WLONG_GRID), d / 4), dim3(WG), 0,
                  stream, x, w, d, order, offsets, long_list, sums, wsums, k, longs);
    if (n > 0) {
        const size_t bytes = sizeof(uint32_t) * (size_t)n;
        if (order_out) AT_HIP(hipMemcpyAsync(order_out, order, bytes, hipMemcpyDeviceToDevice, stream));
        if (sorted_ids_out) AT_HIP(hipMemcpyAsync(sorted_ids_out, sorted_keys, bytes, hipMemcpyDeviceToDevice, stream));
    }
    return AT_OK;
}

}  // namespace

extern "C" {

int at_centroid_accum_weighted_f32(at_ctx* ctx, const float* x, const float* w, int64_t n, int d, const int64_t* ids, int k,
                                   float* sums, float* wsums, uint32_t* order_out, uint32_t* sorted_ids_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx, "at_centroid_accum_weighted_f32: ctx is null");
    AT_REQUIRE(n >= 0 && n < (int64_t)UINT32_MAX && d > 0 && k > 0 && k < (1 << 30),
               "at_centroid_accum_weighted_f32: bad sizes n=%lld d=%d k=%d", (long long)n, d, k);
    AT_REQUIRE(sums && wsums && (n == 0 || (x && w && ids)), "at_centroid_accum_weighted_f32: null pointer");
    AT_HIP(hipSetDevice(ctx->device));
    AT_TRY(at_guard_enter(&ctx->guard[AT_GUARD_WACC], stream));   // calls of one context share the WS_WACC_* slots
    const int rc = waccum_queue(ctx, x, w, (long)n, d, reinterpret_cast<const long*>(ids), k, sums, wsums, order_out,
                                sorted_ids_out, stream);
    const int grc = at_guard_leave(&ctx->guard[AT_GUARD_WACC], stream);
    return rc != AT_OK ? rc : grc;
}

// include/at_debug.h: the sizes at which the weighted accumulation changes its path (NULL skips a field)
int at_waccum_limits(int* short_batch, int* short_batch_wide, int* long_list, int* ring_chunk) {
    if (short_batch) *short_batch = WSHORT_RB;
    if (short_batch_wide) *short_batch_wide = WSHORT_RB_WIDE;
    if (long_list) *long_list = (int)WLONG_LIST;
    if (ring_chunk) *ring_chunk = WLONG_CHUNK;
    return AT_OK;
}

}  // extern "C"
