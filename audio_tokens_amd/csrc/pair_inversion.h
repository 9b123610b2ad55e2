// pair_inversion.h -- the counting sort of (query, probe) pairs by list, once (ivf.hip, ivfpq.hip).
//
// count / offsets / scatter: pair p = query * nprobe + probe slot with a list in [0, nlist) lands somewhere in
// pairtab[pair_start[l] .. pair_start[l + 1]); where exactly is decided by an atomic and does not matter, a query's result
// does not depend on the slot that computes it.  units[l] is the prefix sum of ceil(count / per): the blocks of `per`
// pairs of a search, or the tiles / groups of `per` rows of a build.  list_of_unit finds the list of a block (tile, group)
// by binary search.  A pair without a list gets its k places of the partial lists emptied here.
//
// The kernels sit in an unnamed namespace: every file that includes this header gets its own copies.
#pragma once
#include "at_internal.h"

#if defined(__HIPCC__)

namespace {
namespace pinv {

constexpr int PWG = 256;
constexpr uint64_t PAIR_KEY_NONE = ~(uint64_t)0;   // an empty place of a partial list

// cnt[l] += 1 for every entry l of v in [0, nlist); anything else (-1: no list) is skipped
__global__ void __launch_bounds__(PWG)
ivf_count_kernel(const long* __restrict__ v, long m, int nlist, int* __restrict__ cnt) {
    const long t = (long)blockIdx.x * PWG + threadIdx.x;
    if (t >= m) return;
    const long l = v[t];
    if (l >= 0 && l < nlist) atomicAdd(cnt + l, 1);
}

// start[l] = sum of cnt[0 .. l), units[l] = sum of ceil(cnt / per) over [0 .. l), l = 0 .. nlist; one workgroup, thread
// t owns the lists [t * seg, (t + 1) * seg)
__global__ void __launch_bounds__(PWG)
ivf_offsets_kernel(const int* __restrict__ cnt, int nlist, int per, int* __restrict__ start, int* __restrict__ units) {
    __shared__ int sa[PWG], sb[PWG];
    const int t = threadIdx.x;
    const int seg = (nlist + PWG - 1) / PWG;
    const int l0 = t * seg < nlist ? t * seg : nlist, l1 = l0 + seg < nlist ? l0 + seg : nlist;
    int a = 0, b = 0;
    for (int l = l0; l < l1; l++) {
        a += cnt[l];
        b += (cnt[l] + per - 1) / per;
    }
    sa[t] = a;
    sb[t] = b;
    __syncthreads();
    if (t == 0) {
        int ra = 0, rb = 0;
        for (int i = 0; i < PWG; i++) {
            const int ca = sa[i], cb = sb[i];
            sa[i] = ra;
            sb[i] = rb;
            ra += ca;
            rb += cb;
        }
        start[nlist] = ra;
        units[nlist] = rb;
    }
    __syncthreads();
    a = sa[t];
    b = sb[t];
    for (int l = l0; l < l1; l++) {
        start[l] = a;
        units[l] = b;
        a += cnt[l];
        b += (cnt[l] + per - 1) / per;
    }
}

// the l in [0, nlist) with tab[l] <= b < tab[l + 1]; the caller has checked b < tab[nlist] (tab[0] = 0, tab ascends)
__device__ __forceinline__ int list_of_unit(const int* __restrict__ tab, int nlist, int b) {
    int lo = 0, hi = nlist;   // tab[lo] <= b < tab[hi] throughout
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// pair p with a list: into its list's stretch of pairtab; without one: its k places of the partial lists are empty
__global__ void __launch_bounds__(PWG)
ivf_scatter_kernel(const long* __restrict__ probes, int ptotal, int nlist, const int* __restrict__ pair_start,
                   int* __restrict__ cursor, int* __restrict__ pairtab, uint64_t* __restrict__ partial, int k) {
    const int p = blockIdx.x * PWG + threadIdx.x;
    if (p >= ptotal) return;
    const long l = probes[p];
    if (l >= 0 && l < nlist) {
        // cursor[l] counts the same pairs ivf_count_kernel counted: slot < pair_start[l + 1] <= ptotal
        const int slot = pair_start[l] + atomicAdd(cursor + l, 1);
        if (slot >= 0 && slot < ptotal) pairtab[slot] = p;
    } else {
        for (int s = 0; s < k; s++) partial[(size_t)p * k + s] = PAIR_KEY_NONE;
    }
}

}  // namespace pinv
}  // namespace

#endif
