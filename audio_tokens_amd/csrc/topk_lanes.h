// topk_lanes.h -- the running per-lane top-KL list of the dense sweeps, once (knn.hip, ivf.hip).
//
// A lane of a cs::Sweep (chunked_sweep.h) meets the candidates of its row in ascending index order -- (tile, accumulator,
// register) is ascending for a fixed half-wave -- and keeps the KL smallest (dis, index) in registers, ascending.  A
// finished accumulator gives each lane 16 candidates: offer16 first compares their minimum with every lane's KL-th key
// (one ballot) and then each candidate (one ballot each), so the insert network runs only for candidates that improve
// some lane.  A strict `<` insert that puts a candidate behind its equals keeps the lexicographic (dis, index) order
// without comparing indices.  The two half-waves (same 32 rows, disjoint indices) merge once at the end: the elementwise
// (dis, index)-minimum of one list and the other reversed is a bitonic sequence of the KL smallest, sorted by a bitonic
// merge network.  A candidate that is NaN or +inf never enters (no `<` holds for it): an empty place is (+inf, cs::NONE).
#pragma once
#include "chunked_sweep.h"

#if defined(__HIPCC__)

namespace tk {

// insert (c, id) into the ascending list; entries <= c stay in front of it (the lane's ids ascend)
template <int KL>
__device__ __forceinline__ void topk_insert(float (&ld)[KL], unsigned (&li)[KL], float c, unsigned id) {
#pragma unroll
    for (int s = KL - 1; s > 0; s--) {
        const bool lt_prev = c < ld[s - 1], lt_here = c < ld[s];
        ld[s] = lt_prev ? ld[s - 1] : (lt_here ? c : ld[s]);
        li[s] = lt_prev ? li[s - 1] : (lt_here ? id : li[s]);
    }
    const bool lt0 = c < ld[0];
    ld[0] = lt0 ? c : ld[0];
    li[0] = lt0 ? id : li[0];
}

__device__ __forceinline__ bool lex_less(float da, unsigned ia, float db, unsigned ib) {
    return da < db || (da == db && ia < ib);
}

template <int KL>
__device__ __forceinline__ void clear(float (&ld)[KL], unsigned (&li)[KL]) {
#pragma unroll
    for (int s = 0; s < KL; s++) {
        ld[s] = __builtin_inff();
        li[s] = cs::NONE;
    }
}

// u[4 g + e] = fma(-2, acc[4 g + e], xn + |c|^2) of the 16 registers of a finished accumulator, before the clamp; cnh:
// the norms of the accumulator's 32 rows from this half-wave's first one on (+ 4 h)
__device__ __forceinline__ void l2_of_acc16(const f32x16& acc, const float* cnh, float xn, float (&u)[16]) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const f32x4 cn = *reinterpret_cast<const f32x4*>(cnh + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; e++) u[4 * g + e] = __builtin_fmaf(-2.0f, acc[4 * g + e], xn + cn[e]);
    }
}

// the 16 candidates (clamp0(u[e]), idbase + reg_offset(e)) of a finished accumulator, in ascending index.  Every lane
// of the wave calls it together (ballots).
template <int KL>
__device__ __forceinline__ void offer16(float (&ld)[KL], unsigned (&li)[KL], const float (&u)[16], unsigned idbase) {
    // clamp0(u) < kth only if u < kth (kth >= 0): the minimum decides whether anything can enter
    float m = __builtin_fminf(u[0], u[1]);
#pragma unroll
    for (int e = 2; e < 16; e += 2) m = __builtin_fminf(__builtin_fminf(m, u[e]), u[e + 1]);
    if (__builtin_amdgcn_ballot_w64(m < ld[KL - 1]) != 0) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const float cv = cs::clamp0(u[e]);
            if (__builtin_amdgcn_ballot_w64(cv < ld[KL - 1]) != 0)
                topk_insert<KL>(ld, li, cv, idbase + (unsigned)cs::reg_offset(e));
        }
    }
}

// merge the half-waves: min(A[s], B[KL-1-s]) is bitonic and holds the KL smallest; then sort it.  Both half-waves end
// with the row's list in (cd, ci).
template <int KL>
__device__ __forceinline__ void merge_halves(const float (&ld)[KL], const unsigned (&li)[KL], float (&cd)[KL],
                                             unsigned (&ci)[KL]) {
#pragma unroll
    for (int s = 0; s < KL; s++) {
        const float od = __shfl_xor(ld[KL - 1 - s], 32);
        const unsigned oi = (unsigned)__shfl_xor((int)li[KL - 1 - s], 32);
        const bool take = lex_less(od, oi, ld[s], li[s]);
        cd[s] = take ? od : ld[s];
        ci[s] = take ? oi : li[s];
    }
#pragma unroll
    for (int st = KL / 2; st > 0; st /= 2) {
#pragma unroll
        for (int s = 0; s < KL; s++) {
            if (s & st) continue;
            const bool sw = lex_less(cd[s + st], ci[s + st], cd[s], ci[s]);
            const float td = cd[s];
            const unsigned ti = ci[s];
            cd[s] = sw ? cd[s + st] : cd[s];
            ci[s] = sw ? ci[s + st] : ci[s];
            cd[s + st] = sw ? td : cd[s + st];
            ci[s + st] = sw ? ti : ci[s + st];
        }
    }
}

}  // namespace tk

#endif  // __HIPCC__
