// accum_kernels.h -- the device code that the plain centroid sums (accum.hip) and the weighted ones (waccum.hip) share:
// the sort keys, the segment starts, the one-wave walk of a short member list and the feature-sliced kernel of a long one.
//
// Both contracts are one chain per (cluster, feature) over the members in ASCENDING row, from +0:
//     WEIGHTED = false:  s <- s + x[i][f]                the cluster's count beside the sums
//     WEIGHTED = true:   s <- fmaf(x[i][f], w[i], s)     the chain s <- s + w[i], in the same order, beside them
// Every fused multiply-add is written out as __builtin_fmaf (the library is built with -ffp-contract=off); a product
// rounded before it is added would be another number.  No float atomics: the bits do not depend on the launch.
//
// Everything is in an unnamed namespace: each object compiles its own copy with its own flags.  accum.o instantiates
// the WEIGHTED = false forms only; waccum.o the WEIGHTED = true ones, without packed-fp32 instructions (Makefile,
// NOPK_OBJS; DESIGN.md sections 2b and 6l) -- compiled with accum.o's flags they come out as other code.
#pragma once
#include "at_internal.h"

#define AT_TRY(expr) do { const int rc_ = (expr); if (rc_ != AT_OK) return rc_; } while (0)

namespace {

constexpr int WG = 256;

// The sizes at which a form changes its path.  Lists of up to LONG_LIST members are one wave's walk
// (centroid_accum_kernel), RB / RB_WIDE rows per register set (lanes with 1 or 2 / with 4 features); longer ones are
// cut across features (centroid_accum_long_kernel): CHUNK members per ring buffer, read by the adder in batches of BATCH.
template <bool WEIGHTED>
struct AccumShape {
    static constexpr uint32_t LONG_LIST = WEIGHTED ? 1024 : 2048;
    static constexpr int RB = 16, RB_WIDE = 8;
    static constexpr int CHUNK = WEIGHTED ? 1536 : 2048;
    static constexpr int BATCH = WEIGHTED ? 64 : 128;
    static constexpr int RING_ROWS = WEIGHTED ? 5 : 4;   // the slice's four features (and the weights)
    static constexpr int LOADERS = WG - 64;              // threads that load
    static constexpr int PER_THREAD = (CHUNK + LOADERS - 1) / LOADERS;
    static_assert(CHUNK % BATCH == 0 && BATCH % 16 == 0, "the adder reads the ring in whole batches");
    static_assert(2 * RING_ROWS * CHUNK * sizeof(float) <= 64 * 1024, "the ring is static LDS");
};

__global__ void __launch_bounds__(WG) make_keys_kernel(const long* __restrict__ ids, long n, int k,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const long c = ids[i];
    // an id outside [0, k) (e.g. -1 from an all-NaN row) is parked in a trailing bucket that no centroid reads
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

// offsets[c] = first position p of the sorted keys with keys[p] >= c, for c in [0, k].  With `longs`: the clusters with
// more than long_list members go into longs[1 ..] (any order: it decides which workgroup sums a list, not a bit of the
// sum), longs[0] = how many (zero before the launch).
__global__ void __launch_bounds__(WG) segment_offsets_kernel(const uint32_t* __restrict__ keys, long n, int k,
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
// lane l holds member l's row index, broadcast with readlane when its turn comes -- and, WEIGHTED, its weight, so the
// weight of a row costs the wave one 4-byte load per 64 members and lane.  The weight chain ws is the same value in
// every lane (a vector add of a uniform operand).  Lane 0 of the cluster's first slab stores the count, or ws, in `tail`.
template <int VEC, bool WEIGHTED>
__global__ void __launch_bounds__(WG) centroid_accum_kernel(const float* __restrict__ x, const float* __restrict__ w, int d,
                                                            const uint32_t* __restrict__ order,
                                                            const uint32_t* __restrict__ offsets, int k, int slabs,
                                                            uint32_t long_list, float* __restrict__ sums,
                                                            float* __restrict__ tail) {
    const int lane = threadIdx.x & 63;
    const long wv = (long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (wv >= (long)k * slabs) return;
    const int c = (int)(wv / slabs);
    const int slab = (int)(wv - (long)c * slabs);
    const int f0 = (slab * 64 + lane) * VEC;
    const bool live = f0 < d;  // d is a multiple of VEC
    const uint32_t beg = offsets[c], end = offsets[c + 1];
    if (end - beg > long_list) return;  // left to centroid_accum_long_kernel

    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; v++) acc[v] = 0.0f;
    float ws = 0.0f;

    // Rows are fetched RB at a time into one of two register sets: the loads of batch i+1 are in flight while batch i
    // is added (in member order: one dependent chain per feature, as the contract says), and the indices (and weights)
    // of the next 64 members are fetched while this block of 64 is summed.  A list is one wave's sequential walk, so
    // the kernel lasts as long as its longest lists: what bounds those is how many row reads the wave keeps in flight
    // -- 16 per set (32 in flight) instead of round 2's 8: 168 -> see DESIGN us at 2 M x 64.
    constexpr int RB = VEC == 4 ? AccumShape<WEIGHTED>::RB_WIDE : AccumShape<WEIGHTED>::RB;
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
                if constexpr (WEIGHTED) {
                    const float wt = __uint_as_float(__builtin_amdgcn_readlane(wmine, (m + u) & 63));
#pragma unroll
                    for (int v = 0; v < VEC; v++) acc[v] = __builtin_fmaf(t[u][v], wt, acc[v]);
                    ws = ws + wt;
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; v++) acc[v] += t[u][v];
                }
            }
        }
    };
    auto members = [&](uint32_t base, uint32_t* mine, uint32_t* wmine) {   // (base < end)
        const bool have = lane < min(64u, end - base);
        *mine = have ? order[base + lane] : 0u;
        if constexpr (WEIGHTED) *wmine = have ? __float_as_uint(w[*mine]) : 0u;
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
    if (slab == 0 && lane == 0) tail[c] = WEIGHTED ? ws : (float)(end - beg);
}

// N consecutive members of an adder lane's ring row `src` (and of the weight row `wr`) onto its chain: all the 16-byte
// LDS reads first, so that their latency is paid once per N members.  `plain` is the lane of the weight chain: its
// row holds the weights themselves, times one.  (The ternary stays inside the fmaf's argument: there the compiler
// skips that lane's weight reads; with the weight selected ahead of the call it puts a v_cndmask before every fmaf.)
template <bool WEIGHTED, int N>
__device__ __forceinline__ float ring_batch(const float* src, const float* wr, bool plain, float acc) {
    float4 t[N / 4], q[N / 4];
#pragma unroll
    for (int u = 0; u < N / 4; u++) {
        t[u] = *reinterpret_cast<const float4*>(src + 4 * u);
        if constexpr (WEIGHTED) q[u] = *reinterpret_cast<const float4*>(wr + 4 * u);
    }
#pragma unroll
    for (int u = 0; u < N / 4; u++) {
        if constexpr (WEIGHTED) {
            acc = __builtin_fmaf(t[u].x, plain ? 1.0f : q[u].x, acc);
            acc = __builtin_fmaf(t[u].y, plain ? 1.0f : q[u].y, acc);
            acc = __builtin_fmaf(t[u].z, plain ? 1.0f : q[u].z, acc);
            acc = __builtin_fmaf(t[u].w, plain ? 1.0f : q[u].w, acc);
        } else {
            acc += t[u].x;
            acc += t[u].y;
            acc += t[u].z;
            acc += t[u].w;
        }
    }
    return acc;
}

// Long member lists (one huge cluster, e.g. every digital-silence frame) would leave a single wavefront chasing HBM
// latency for milliseconds.  The sums of different features are independent, so such a cluster is cut ACROSS FEATURES:
// one workgroup per (long cluster, 4-feature slice).  Waves 1-3 stream that 16-byte slice of every member row (and the
// member's weight), in member order, into a double-buffered feature-major LDS ring (all index loads, then all row and
// weight loads, then the LDS writes, so a whole chunk is in flight at once); four lanes of wave 0 do nothing but the
// dependent chain of their feature.  Same ascending-member order, hence the same bits, as the one-wave kernel.
// WEIGHTED: five lanes.  Lanes 0-3 run acc <- fmaf(x, w, acc) (the product is never rounded: the weights ride in a ring
// row of their own and meet the rows in the adder), lane 4 the weight chain, written as fmaf(w, 1, acc) so that the
// five lanes execute one instruction stream -- w * 1 is exact, hence the single rounding of acc + w.
//
// early != 0: list `slot` of the early lists (at most EARLY_MAX of them: cluster cluster_of[slot], members offsets[slot]
// ..); marks the cluster done[c] = gen.  early == 0, list mode: the workgroups stride over the slots [slot0, slot1) of cluster_of (cluster_of[0]
// = its length, the clusters behind it), offsets indexed by cluster.  `tail` gets the count, or the weight sum.
constexpr int EARLY_MAX = 16;       // long clusters whose member lists come from accum.hip's ordered compaction

template <bool WEIGHTED>
__global__ void __launch_bounds__(WG) centroid_accum_long_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 int d, const uint32_t* __restrict__ order,
                                                                 const uint32_t* __restrict__ offsets,
                                                                 uint32_t long_list, float* __restrict__ sums,
                                                                 float* __restrict__ tail, int k, int early,
                                                                 const int* __restrict__ cluster_of,
                                                                 const int* __restrict__ n_slots,
                                                                 unsigned* __restrict__ done, unsigned gen, int slot0,
                                                                 int slot1) {
    using S = AccumShape<WEIGHTED>;
    constexpr int CHUNK = S::CHUNK, PER_THREAD = S::PER_THREAD, LOADERS = S::LOADERS;
    // feature-major ring: ring[buffer][row][member], so an adder lane reads four consecutive members of its row with
    // one 16-byte LDS read; rows 0-3 the slice's features, row 4 the weights
    __shared__ __attribute__((aligned(16))) float ring[2][S::RING_ROWS][CHUNK];
    const int n_slot = min(early ? min(*n_slots, EARLY_MAX) : cluster_of[0], slot1);
    const int piece = blockIdx.y;  // features 4*piece .. 4*piece+3
    for (int slot = slot0 + blockIdx.x; slot < n_slot; slot += gridDim.x) {
        const int c = early ? cluster_of[slot] : cluster_of[1 + slot];
        if (c < 0 || c >= k) continue;
        const uint32_t beg = early ? offsets[slot] : offsets[c], end = early ? offsets[slot + 1] : offsets[c + 1];
        const uint32_t len = end - beg;
        if (len <= long_list) continue;  // uniform for the workgroup
        const int tid = threadIdx.x;
        const bool adder = tid < 64;
        const uint32_t nchunks = (len + CHUNK - 1) / CHUNK;
        const float4* rows = reinterpret_cast<const float4*>(x) + piece;
        const int d4 = d >> 2;

        auto stage = [&](uint32_t ch) {  // loaders only
            const uint32_t m0 = ch * CHUNK;
            const uint32_t cnt = min((uint32_t)CHUNK, len - m0);
            const uint32_t t = tid - 64;
            uint32_t src[PER_THREAD];
            float4 v[PER_THREAD];
            [[maybe_unused]] float wt[PER_THREAD];
#pragma unroll
            for (int u = 0; u < PER_THREAD; u++) {
                const uint32_t e = t + u * LOADERS;
                src[u] = e < cnt ? order[beg + m0 + e] : 0u;
            }
#pragma unroll
            for (int u = 0; u < PER_THREAD; u++) {
                const uint32_t e = t + u * LOADERS;
                v[u] = e < cnt ? rows[(size_t)src[u] * d4] : make_float4(0, 0, 0, 0);
                if constexpr (WEIGHTED) wt[u] = e < cnt ? w[src[u]] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < PER_THREAD; u++) {
                const uint32_t e = t + u * LOADERS;
                if (e < cnt) {
                    ring[ch & 1][0][e] = v[u].x;
                    ring[ch & 1][1][e] = v[u].y;
                    ring[ch & 1][2][e] = v[u].z;
                    ring[ch & 1][3][e] = v[u].w;
                    if constexpr (WEIGHTED) ring[ch & 1][4][e] = wt[u];
                }
            }
        };

        float acc = 0.0f;
        if (!adder) stage(0);
        __syncthreads();
        for (uint32_t ch = 0; ch < nchunks; ch++) {
            if (!adder) {
                if (ch + 1 < nchunks) stage(ch + 1);
            } else if (tid < S::RING_ROWS) {
                const float* src = ring[ch & 1][tid];
                const float* wr = ring[ch & 1][S::RING_ROWS - 1];
                const bool plain = tid == 4;
                const uint32_t cnt = min((uint32_t)CHUNK, len - ch * CHUNK);
                // one dependent chain; the LDS latency is paid once per batch (unweighted, on a 46 000-member list:
                // batches of 16 380 us, of 128 310 us)
                uint32_t m = 0;
                for (; m + S::BATCH <= cnt; m += S::BATCH) acc = ring_batch<WEIGHTED, S::BATCH>(src + m, wr + m, plain, acc);
                for (; m + 16 <= cnt; m += 16) acc = ring_batch<WEIGHTED, 16>(src + m, wr + m, plain, acc);
                for (; m < cnt; m++) acc = WEIGHTED ? __builtin_fmaf(src[m], plain ? 1.0f : wr[m], acc) : acc + src[m];
            }
            __syncthreads();
        }
        if (tid < 4) sums[(size_t)c * d + 4 * piece + tid] = acc;
        if constexpr (WEIGHTED) {
            if (tid == 4 && piece == 0) tail[c] = acc;
        } else if (tid == 0 && piece == 0) {
            tail[c] = (float)len;
            if (early && done) done[c] = gen;
        }
        __syncthreads();   // (the ring is reused by the next list)
    }
}

}  // namespace
