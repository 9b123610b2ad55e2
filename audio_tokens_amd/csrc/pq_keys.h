// pq_keys.h -- the key-ordered candidate buffer of the scans over product-quantiser codes, once (pq_search.hip,
// ivfpq.hip).
//
// key = (distance bits << 32) | id orders (distance, id) lexicographically for distances >= +0 below +inf.  A scan keeps,
// per query, up to CAP - 2 waiting keys in LDS and a threshold key in registers; when a round of WG rows could overflow
// the buffer it is sorted (bitonic, the whole workgroup) and cut to the k smallest, whose last becomes the threshold
// (pq_search.hip's header says the rest).  The merge kernel streams the partial lists of one query through the same
// buffer.  Piece / piece_byte: a code row in loads of 16, 8, 4 or 1 bytes.
//
// Everything sits in an unnamed namespace: every file that includes this header gets its own copies.
#pragma once
#include "at_internal.h"

#if defined(__HIPCC__)

namespace {
namespace pqk {

constexpr int WG = 256;
constexpr int CAP = 2 * WG;          // places per query in LDS: CAP - 2 candidate keys, the last two hold the round counters
constexpr int FULL_AT = CAP - 2 - WG;   // more keys than this in front of a round: a round may add WG, so sort and cut first
constexpr int MAX_K = 128;           // k <= FULL_AT, and half of it leaves the sorts rare
constexpr int MAX_M = 64;            // the tables of two queries in 128 KiB
constexpr int QB_WIDE_MAX_M = 32;    // up to here four queries per workgroup
constexpr uint64_t KEY_NONE = ~(uint64_t)0;
constexpr uint64_t KEY_LIMIT = (uint64_t)0x7f800000u << 32;   // the keys below it have a distance below +inf

__host__ __device__ inline int queries_per_block(int M) { return M <= QB_WIDE_MAX_M ? 4 : 2; }

// buf[0 .. cnt) ascending, by every thread of the workgroup; cnt <= CAP is the same in all of them.  The bitonic network
// in its form with every comparison ascending (the first step of a merge pairs i with its mirror image in the block):
// the places from cnt up to the next power of two count as all-ones keys, which no comparison would move, so they are
// neither read nor written.  Ends behind a barrier.
__device__ void sort_keys(uint64_t* buf, int cnt) {
    const int t = threadIdx.x;
    int P = 2;
    while (P < cnt) P <<= 1;
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int i = 2 * t - (t & (stride - 1));
            const int j = 2 * stride == size ? (i | (size - 1)) - (i & (stride - 1)) : i + stride;
            if (j < cnt) {   // (i < j; t < P / 2 follows from it)
                const uint64_t a = buf[i], b = buf[j];
                if (a > b) {
                    buf[i] = b;
                    buf[j] = a;
                }
            }
            __syncthreads();
        }
}

// the k smallest of buf[0 .. cnt) to the front, the k-th as the new threshold (every thread reads it for itself: the
// appends that follow go behind it); returns the keys kept
__device__ int cut_to_k(uint64_t* buf, uint64_t& thr, int cnt, int k) {
    sort_keys(buf, cnt);
    if (cnt >= k) {
        thr = buf[k - 1];
        cnt = k;
    }
    return cnt;
}

template <int W> struct Piece;
template <> struct Piece<16> { typedef uint4 type; };
template <> struct Piece<8> { typedef uint2 type; };
template <> struct Piece<4> { typedef unsigned type; };
template <> struct Piece<1> { typedef uint8_t type; };

template <int W>
__device__ __forceinline__ unsigned piece_byte(const typename Piece<W>::type& v, int b) {
    if constexpr (W == 16) {
        const unsigned w = b < 4 ? v.x : b < 8 ? v.y : b < 12 ? v.z : v.w;
        return (w >> (8 * (b & 3))) & 255u;
    } else if constexpr (W == 8) {
        const unsigned w = b < 4 ? v.x : v.y;
        return (w >> (8 * (b & 3))) & 255u;
    } else if constexpr (W == 4) {
        return (v >> (8 * b)) & 255u;
    } else {
        return v;
    }
}

// one workgroup per query: the k smallest of its `total` listed keys (KEY_NONE: an empty place)
__global__ void __launch_bounds__(WG)
pq_merge_kernel(const uint64_t* __restrict__ lists, long total, int k, long* __restrict__ ids, float* __restrict__ dist) {
    __shared__ uint64_t buf[CAP];
    __shared__ int add[3];
    const int tid = threadIdx.x;
    uint64_t thr = KEY_LIMIT;
    const uint64_t* src = lists + (long)blockIdx.x * total;
    if (tid < 3) add[tid] = 0;
    __syncthreads();
    int base = 0, cur = 0;
    for (long r0 = 0; r0 < total; r0 += WG) {
        const int nxt = cur == 2 ? 0 : cur + 1;
        if (tid == 0) add[nxt] = 0;
        if (r0 + tid < total) {
            const uint64_t key = src[r0 + tid];
            if (key < thr) buf[base + atomicAdd(&add[cur], 1)] = key;
        }
        __syncthreads();
        base += add[cur];
        if (base > FULL_AT) base = cut_to_k(buf, thr, base, k);
        cur = nxt;
    }
    sort_keys(buf, base);
    const int cnt = base < k ? base : k;
    for (int t = tid; t < k; t += WG) {
        const uint64_t key = t < cnt ? buf[t] : KEY_NONE;
        const long o = (long)blockIdx.x * k + t;
        ids[o] = t < cnt ? (long)(uint32_t)key : -1;
        if (dist) dist[o] = t < cnt ? __uint_as_float((uint32_t)(key >> 32)) : __builtin_inff();
    }
}

// an empty index: every place is (-1, +inf)
__global__ void __launch_bounds__(WG)
pq_nothing_kernel(long total, long* __restrict__ ids, float* __restrict__ dist) {
    const long t = (long)blockIdx.x * WG + threadIdx.x;
    if (t >= total) return;
    ids[t] = -1;
    if (dist) dist[t] = __builtin_inff();
}

}  // namespace pqk
}  // namespace

#endif
