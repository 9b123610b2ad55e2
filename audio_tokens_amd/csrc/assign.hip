// assign.hip -- nearest centroid under squared L2 on gfx950 (at_assign_f32).
//
// Replaces faiss.IndexFlatL2.search(x, 1) at processors/spec_tokenizer.py:77 and inside
// faiss.Kmeans.train (processors/cluster_creator.py:54-56) of danavery/audio-tokens.
//
// Arithmetic contract (identical to oracle/oracle.c orc_assign, bit for bit):
//   ip(i,j)  = fmaf chain over the feature index, ascending, from +0   (v_mfma_f32_32x32x2_f32)
//   xn(i), cn(j) likewise with both operands equal
//   dis(i,j) = max(0, (xn + cn) - 2*ip)            one rounding for the add, one for the fma
//   ids[i]   = lowest j with minimal dis, dist[i] = that dis
//   A centroid is a candidate only with dis < +inf (the strict '<' from +inf): a row none of whose distances is
//   finite -- |x|^2 overflows from finite elements -- is (-1, +inf) on every route, whatever it was hinted; a
//   centroid whose |c|^2 is +inf is never named.  The dense epilogue has this from its compare; the hinted and
//   pruned sweeps, whose exact update breaks ties by index, from no_winner() where store_answer() writes the row.
//
// Data flow.  The centroid table is re-laid once per call into tiles of 32*NA centroids whose rows
// are already in LDS order (k split even/odd per 8 features so that one ds_read_b128 feeds four
// consecutive MFMA k-steps, 16-byte chunks XOR-swizzled by row so the reads are conflict free),
// each tile followed by its squared norms.  A workgroup of 4 waves streams every tile through a
// double-buffered LDS copy while each wave keeps its 32*NB rows of x in registers for the whole
// sweep (B operand: lane l holds x[row l&31][k = 2s + (l>>5)]); the 32x32 accumulator puts the x
// row on the lane and 16 centroids in the registers, so the running arg-min is lane-local and the
// two half-waves are merged once at the end.  The arg-min of a finished accumulator is scheduled
// between the MFMAs of the next one, including across the tile boundary (the last accumulator of
// a tile is carried into the next loop iteration).  HBM traffic: x once (4d B/row) + 12 B/row out;
// the centroid image (k*d*4 B) is L2/Infinity-Cache resident.  Bound: fp32 MFMA (2*d*k flop/row).
//
// Layout of this file.  Five MFMA sweeps share one arithmetic: assign_mfma_kernel (dense, d = 64 / 128),
// assign_mfma_hinted_kernel, assign_mfma_pruned_kernel (LDS-DMA) and assign_mfma_pruned_reg_kernel (register-staged),
// assign_mfma_anyd_kernel (any d % 4 == 0).  Each step of that arithmetic is written once, above the kernels ("The
// steps that the MFMA sweeps share"; the layout functions, the x chunk, the half-wave merge and the 1 KiB DMA come from
// chunked_sweep.h), and a kernel body is its schedule: what it stages, when it prefetches, when it finishes an
// accumulator.  Where a kernel keeps a step written out, a comment there says what the shared form cost it.
#include <cstdlib>

#include "at_internal.h"
#include "chunked_sweep.h"

namespace {

constexpr int WG = 256;    // threads per workgroup (4 waves)
using cs::CN_PAD;      // floats reserved per tile for the squared norms (whole 1 KiB pieces)
using cs::DC;          // features per chunk of the any-d image (chunked_sweep.h)
using cs::dma_1k;
using cs::tile_rows;
__host__ __device__ constexpr int tile_floats(int dp, int na) { return tile_rows(na) * dp + CN_PAD; }

// ---------------------------------------------------------------------------------------------
// Centroid image: tile t holds rows t*R .. t*R+R-1 (R = 32*na).  Row r, 16-byte chunk pc
// (physical) holds logical chunk lc = pc ^ (r & 15); lc = 2q + h holds features 8q + {0,2,4,6} + h.
// Features >= d and rows >= k are zero; |c|^2 of a row >= k is +inf so it can never win.
//
// (cs::image_slot / cs::image_norm, chunked_sweep.h: the producers of every image share them.)
using cs::image_norm;
using cs::image_slot;

__global__ void __launch_bounds__(WG) prep_centroids_kernel(const float* __restrict__ c, int k, int d,
                                                            int dp, int na, float* __restrict__ img) {
    const int t = blockIdx.x;
    const int R = tile_rows(na);
    float* out = img + (size_t)t * tile_floats(dp, na);
    const int chunks_per_row = dp / 4;
    for (int e = threadIdx.x; e < R * chunks_per_row; e += WG) {
        const int r = e / chunks_per_row, pc = e % chunks_per_row;
        const int row = t * R + r;
        *reinterpret_cast<f32x4*>(out + (size_t)r * dp + pc * 4) =
            image_slot(row < k ? c + (size_t)row * d : nullptr, d, 0, r, pc);
    }
    for (int r = threadIdx.x; r < CN_PAD; r += WG) {
        const int row = t * R + r;
        out[R * dp + r] = image_norm(r < R && row < k ? c + (size_t)row * d : nullptr, d);
    }
}

// The exact update of the hinted and pruned sweeps accepts a lower index on an EQUAL distance, +inf included, and a
// running best without a finite distance starts at +inf: a row none of whose distances is finite (|x|^2 overflows)
// would end with the lowest index its sweep visited.  The contract's strict '<' from +inf never names a centroid at
// +inf, so such a row is (-1, +inf) -- decided once, where the answer is stored, not in the sweep.
__device__ __forceinline__ bool no_winner(unsigned fi, float fd) { return fi == 0xffffffffu || !(fd < __builtin_inff()); }

// One arg-min step with the compare mask kept in VCC (three VALU ops, no SGPR pair to carry):
//   keep = !(dis < bd);  bd = keep ? bd : dis;  br = keep ? br : R
template <int R>
__device__ __forceinline__ void argmin_step(float& bd, unsigned& br, float dis) {
    asm("v_cmp_nlt_f32 vcc, %2, %0\n\t"
        "v_cndmask_b32 %0, %2, %0, vcc\n\t"
        "v_cndmask_b32 %1, %3, %1, vcc"
        : "+v"(bd), "+v"(br)
        : "v"(dis), "n"(R)
        : "vcc");
}

// (xn + cn) - 2*ip of accumulator register r, the contract's distance before its clamp: one rounding for the add, one
// for the fma.  cnv: the lane's 16 norms (load_norms16).
__device__ __forceinline__ float dist_unclamped(const f32x16& acc, int r, float xn, const f32x4 (&cnv)[4]) {
    return __builtin_fmaf(-2.0f, acc[r], xn + cnv[r >> 2][r & 3]);
}

// dis = max(0, (xn + cn) - 2*ip) for accumulator register R, then the arg-min step.
template <int R>
__device__ __forceinline__ void epilogue_from(float& bd, unsigned& br, const f32x16& acc, float xn,
                                              const f32x4 (&cnv)[4]) {
    if constexpr (R < 16) {
        argmin_step<R>(bd, br, __builtin_fmaxf(dist_unclamped(acc, R, xn, cnv), 0.0f));
        epilogue_from<R + 1>(bd, br, acc, xn, cnv);
    }
}

// Running arg-min over one finished accumulator (this lane's 16 centroids, ascending index).
__device__ __forceinline__ void epilogue16(float& bestd, unsigned& bestc, const f32x16& acc, float xn,
                                           const f32x4 (&cnv)[4], unsigned codebase) {
    float bd = bestd;
    unsigned br = 16u;  // 16 = "no improvement from this accumulator"
    epilogue_from<0>(bd, br, acc, xn, cnv);
    bestd = bd;
    bestc = br != 16u ? (codebase | br) : bestc;
}

// Speculative form: the 16 unclamped distances and their minimum cost 2.5 VALU per element; the
// exact 4-op update (clamp, compare, two selects) runs only when some lane of the wave improves
// (a clamped distance can beat bestd only if the unclamped one does, since bestd >= 0).
template <int R>
__device__ __forceinline__ void update_from(float& bd, unsigned& br, const float (&dis)[16]) {
    if constexpr (R < 16) {
        argmin_step<R>(bd, br, __builtin_fmaxf(dis[R], 0.0f));
        update_from<R + 1>(bd, br, dis);
    }
}

__device__ __forceinline__ void epilogue16_spec(float& bestd, unsigned& bestc, const f32x16& acc, float xn,
                                                const f32x4 (&cnv)[4], unsigned codebase) {
    float dis[16];
#pragma unroll
    for (int r = 0; r < 16; r++) dis[r] = dist_unclamped(acc, r, xn, cnv);
    float m = __builtin_fminf(dis[0], dis[1]);
#pragma unroll
    for (int r = 2; r < 16; r += 2) m = __builtin_fminf(__builtin_fminf(m, dis[r]), dis[r + 1]);
    if (__builtin_amdgcn_ballot_w64(m < bestd) != 0) {
        float bd = bestd;
        unsigned br = 16u;
        update_from<0>(bd, br, dis);
        bestd = bd;
        bestc = br != 16u ? (codebase | br) : bestc;
    }
}

// ---------------------------------------------------------------------------------------------
// The steps that the MFMA sweeps below share, once each.  j = lane & 31 is the lane's x row (the accumulator column),
// h = lane >> 5 the k of each MFMA k-pair that the lane feeds.  A sweep differs from its siblings in what it stages,
// when it prefetches and when it finishes an accumulator: that schedule is the kernel's body, the arithmetic is here.

// Row xrow of D features as the B operand of half-wave h (xv[i] = feature 2 i + h); returns |x|^2, the ascending fmaf
// chain.  (The hinted sweep has |x|^2 from the three chains of its guess and drops this one.)
template <int D>
__device__ __forceinline__ float load_x_row(const float* xrow, int h, float (&xv)[D / 2]) {
    const f32x4* p = reinterpret_cast<const f32x4*>(xrow);
    float nrm = 0.0f;
#pragma unroll
    for (int q = 0; q < D / 8; q++) {
        const f32x4 u = p[2 * q], v = p[2 * q + 1];
#pragma unroll
        for (int e = 0; e < 4; e++) nrm = __builtin_fmaf(u[e], u[e], nrm);
#pragma unroll
        for (int e = 0; e < 4; e++) nrm = __builtin_fmaf(v[e], v[e], nrm);
        xv[4 * q + 0] = h ? u[1] : u[0];
        xv[4 * q + 1] = h ? u[3] : u[2];
        xv[4 * q + 2] = h ? v[1] : v[0];
        xv[4 * q + 3] = h ? v[3] : v[2];
    }
    return nrm;
}

// The A fragments of the lane's centroid row, fragment q = features 8 q + {0, 2, 4, 6} + h: read from the swizzled row
// (in LDS; pruned_reg reads the image itself), or already in registers (pruned_reg loads them a group ahead).
struct SwizzledRow {
    const float* row;
    int j, h;
    __device__ __forceinline__ f32x4 operator()(int q) const {
        return *reinterpret_cast<const f32x4*>(row + cs::chunk_slot(j, q, h) * 4);
    }
};
template <int NQ>
struct RegRow {
    const f32x4 (&av)[NQ];
    __device__ __forceinline__ f32x4 operator()(int q) const { return av[q]; }
};

// acc += fragment q of 32 centroid rows x features 8 q .. 8 q + 7 of 32 x rows: four MFMAs, k ascending in the feature
// index.  (The loop over q stays in the kernels: unrolled in here, ahead of the kernel's own loops, the compiler lifts the
// LDS reads out of the row-block loop and hinted<64, 2, 4> grows from 162 to 198 registers.)
template <typename A, int NX>
__device__ __forceinline__ void mfma_fragment(f32x16& acc, const A& afrag, int q, const float (&xv)[NX]) {
    const f32x4 av = afrag(q);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], xv[4 * q + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], xv[4 * q + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], xv[4 * q + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], xv[4 * q + 3], acc, 0, 0, 0);
}

// |c|^2 of the lane's 16 accumulator rows, 8 g + 4 h + (0..3); cnh: the norm of the half-wave's first row (+ 4 h)
__device__ __forceinline__ void load_norms16(const float* cnh, f32x4 (&cnv)[4]) {
#pragma unroll
    for (int g = 0; g < 4; g++) cnv[g] = *reinterpret_cast<const f32x4*>(cnh + 8 * g);
}

// A finished accumulator of a sweep that starts from a guess (hinted, pruned).  The minimum of the 16 unclamped
// distances costs 2.5 VALU per element instead of 6 (nothing kept: the rare exact update recomputes them from the
// accumulator); a clamped distance can tie or beat the running best (>= 0) only if the unclamped one does.
__device__ __forceinline__ float min16_unclamped(const f32x16& acc, float xn, const f32x4 (&cnv)[4]) {
    float m = __builtin_inff();
#pragma unroll
    for (int r = 0; r < 16; r += 2)
        m = __builtin_fminf(__builtin_fminf(m, dist_unclamped(acc, r, xn, cnv)), dist_unclamped(acc, r + 1, xn, cnv));
    return m;
}

// The order of the exact update: lexicographic in (distance, index), so that the answer is the brute-force arg-min with
// lowest-index ties whatever the guess was.  (By value: on references the && stays a branch per register.)
__device__ __forceinline__ bool lex_better(float dd, unsigned idx, float bd, unsigned bi) {
    return dd < bd || (dd == bd && idx < bi);
}

// The pruned sweeps' update: entered only when some lane of the wave needs it; tab: the index table in the group's pad
// (+ 4 h), which maps the half-wave's image rows back to centroids.
__device__ __forceinline__ void lex_update16(float& bestd, unsigned& besti, const f32x16& acc, float xn,
                                             const f32x4 (&cnv)[4], const unsigned* tab) {
    if (__builtin_amdgcn_ballot_w64(min16_unclamped(acc, xn, cnv) <= bestd) != 0) {
        float bd = bestd;
        unsigned bi = besti;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float dd = __builtin_fmaxf(dist_unclamped(acc, r, xn, cnv), 0.0f);
            const unsigned idx = tab[cs::reg_offset(r)];
            const bool better = lex_better(dd, idx, bd, bi);
            bd = better ? dd : bd;
            bi = better ? idx : bi;
        }
        bestd = bd;
        besti = bi;
    }
}

// The answer of one row: the two half-waves (same rows, disjoint centroids) merged and, by the lanes with `mine` (half-wave
// 0, row < n), stored at `row`.  fi is a centroid index: the dense sweeps come with cs::index_of(code, h).
__device__ __forceinline__ void store_answer(float fd, unsigned fi, long row, bool mine, long* ids, float* dist) {
    cs::merge_halves_min(fd, fi);
    if (mine) {
        ids[row] = no_winner(fi, fd) ? -1L : (long)fi;
        if (dist) dist[row] = fd;
    }
}

// What a wave of the pruned sweeps holds for its 32 NB rows (positions pos0 .. of the visiting order): the rows as
// the B operand, the running best from the pre-pass's exact distance to the guess, and the rows' mask words over the
// 32-centroid groups in scalar registers (ng <= 512).
template <int D, int NB>
struct PrunedRows {
    static constexpr int MAXW = 16;  // mask words kept in scalar registers
    float xr[NB][D / 2];
    float xn[NB];
    float bestd[NB];
    unsigned besti[NB];
    long rowid[NB];
    uint32_t mw[NB][MAXW];
    uint32_t any[MAXW];
    int ng, ngw;

    __device__ __forceinline__ PrunedRows(const float* X, long n, const uint32_t* order,
                                          const uint32_t* hint_sorted, const float* bd_in,
                                          const uint32_t* mask, int ng_, int ngw_, long pos0, int j, int h)
        : ng(ng_), ngw(ngw_) {
        const long ntile32 = (n + 31) / 32;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            long pos = pos0 + 32 * b + j;
            if (pos >= n) pos = n - 1;
            const long r = (long)order[pos];
            rowid[b] = r;
            xn[b] = load_x_row<D>(X + r * D, h, xr[b]);
            bestd[b] = bd_in[pos];
            besti[b] = bestd[b] < __builtin_inff() ? hint_sorted[pos] : 0xffffffffu;
            const long tile = pos0 / 32 + b;
#pragma unroll
            for (int w = 0; w < MAXW; w++) {
                uint32_t m = 0;
                if (w < ngw && tile < ntile32) m = mask[(size_t)tile * ngw + w];
                mw[b][w] = __builtin_amdgcn_readfirstlane(m);
            }
        }
#pragma unroll
        for (int w = 0; w < MAXW; w++) {
            any[w] = 0;
#pragma unroll
            for (int b = 0; b < NB; b++) any[w] |= mw[b][w];
        }
    }

    static __device__ __forceinline__ uint32_t word_of(const uint32_t (&m)[MAXW], int w) {
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < MAXW; i++)
            if (i == w) v = m[i];
        return v;
    }
    // first group >= from that some row tile of the wave needs, or ng
    __device__ __forceinline__ int next_group(int from) const {
        int w = from >> 5;
        if (w >= ngw) return ng;
        uint32_t bits = word_of(any, w) & (0xffffffffu << (from & 31));
        while (bits == 0) {
            if (++w >= ngw) return ng;
            bits = word_of(any, w);
        }
        const int g = (w << 5) + __builtin_ctz(bits);
        return g < ng ? g : ng;
    }
    // does row tile b need group g (wave-uniform)
    __device__ __forceinline__ bool needs(int b, int g) const { return (word_of(mw[b], g >> 5) & (1u << (g & 31))) != 0u; }
};

// ---------------------------------------------------------------------------------------------
template <int D, int NB, int NA, bool DMA, int WAVES_PER_SIMD, bool SPEC = false>
__global__ void __launch_bounds__(WG, WAVES_PER_SIMD)
assign_mfma_kernel(const float* __restrict__ X, long n, const float* __restrict__ img, int ntiles,
                   long* __restrict__ ids, float* __restrict__ dist) {
    constexpr int R = tile_rows(NA);
    constexpr int TILE_F = tile_floats(D, NA);
    constexpr int NV = TILE_F / 4;               // float4 per tile image
    constexpr int VPT = (NV + WG - 1) / WG;      // float4 staged per thread (register staging)
    constexpr int PIECES = TILE_F / 256;         // 1 KiB pieces per tile (DMA staging)
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 2 * TILE_F floats

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31;   // x row within a 32-row tile == accumulator column
    const int h = lane >> 5;   // which k of each MFMA k-pair this lane feeds
    const long row0 = ((long)blockIdx.x * 4 + wave) * (32 * NB);

    // ---- x rows -> registers (B operand), |x|^2 as the ascending fmaf chain ----
    float xr[NB][D / 2];
    float xn[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        long r = row0 + 32 * b + j;
        if (r >= n) r = n - 1;
        xn[b] = load_x_row<D>(X + r * D, h, xr[b]);
    }

    float bestd[NB];
    unsigned bestc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        bestd[b] = __builtin_inff();
        bestc[b] = 0xffffffffu;
    }

    // ---- stage tile 0 ----
    // (the staging stays a lambda in this kernel and in the hinted one: as a shared function it cost both 0.5 to 0.9 %
    // at d = 64, profiles/assign_steps_time.jsonl; the pruned and the any-d sweep stage other units anyway)
    auto stage_tile = [&](int tile, float* dst) {
        const float* src = img + (size_t)tile * TILE_F;
#pragma unroll
        for (int p0 = 0; p0 < PIECES; p0 += 4) {
            const int p = p0 + wave;
            if (p < PIECES) dma_1k(src + p * 256 + lane * 4, dst + p * 256);
        }
    };
    f32x4 pf[DMA ? 1 : VPT];
    if constexpr (DMA) {
        stage_tile(0, smem);
    } else {
        const f32x4* src = reinterpret_cast<const f32x4*>(img);
#pragma unroll
        for (int v = 0; v < VPT; v++) {
            const int e = tid + v * WG;
            if (e < NV) reinterpret_cast<f32x4*>(smem)[e] = src[e];
        }
    }
    __syncthreads();

    // the last accumulator of a tile is finished inside the next iteration
    f32x16 accP = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f32x4 cnP[4];
#pragma unroll
    for (int g = 0; g < 4; g++) cnP[g] = {__builtin_inff(), __builtin_inff(), __builtin_inff(), __builtin_inff()};
    unsigned codeP = 0u;

    for (int ct = 0; ct < ntiles; ct++) {
        const float* cur = smem + (ct & 1) * TILE_F;
        const bool more = ct + 1 < ntiles;
        if (more) {
            if constexpr (DMA) {
                stage_tile(ct + 1, smem + ((ct + 1) & 1) * TILE_F);
            } else {
                const f32x4* src = reinterpret_cast<const f32x4*>(img + (size_t)(ct + 1) * TILE_F);
#pragma unroll
                for (int v = 0; v < VPT; v++) {
                    const int e = tid + v * WG;
                    if (e < NV) pf[v] = src[e];
                }
            }
        }

#pragma unroll
        for (int a = 0; a < NA; a++) {
            f32x4 cnv[4];
            load_norms16(cur + R * D + a * 32 + 4 * h, cnv);
            const SwizzledRow arow{cur + (a * 32 + j) * D, j, h};
            const unsigned codebase = (unsigned)(ct * NA + a) * 16u;
#pragma unroll
            for (int b = 0; b < NB; b++) {
                f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < D / 8; q++) mfma_fragment(acc, arow, q, xr[b]);
                if constexpr (SPEC) {
                    epilogue16_spec(bestd[b], bestc[b], acc, xn[b], cnv, codebase);
                    continue;
                }
                if (a == 0 && b == 0)  // previous tile's last accumulator (no-op on the first tile)
                    epilogue16(bestd[NB - 1], bestc[NB - 1], accP, xn[NB - 1], cnP, codeP);
                if (a == NA - 1 && b == NB - 1) {
                    accP = acc;
#pragma unroll
                    for (int g = 0; g < 4; g++) cnP[g] = cnv[g];
                    codeP = codebase;
                } else {
                    epilogue16(bestd[b], bestc[b], acc, xn[b], cnv, codebase);
                }
            }
        }

        if constexpr (!DMA) {
            if (more) {
                f32x4* dst = reinterpret_cast<f32x4*>(smem + ((ct + 1) & 1) * TILE_F);
#pragma unroll
                for (int v = 0; v < VPT; v++) {
                    const int e = tid + v * WG;
                    if (e < NV) dst[e] = pf[v];
                }
            }
        }
        __syncthreads();  // (with LDS-DMA in flight hipcc makes this vmcnt(0) + s_barrier)
    }
    epilogue16(bestd[NB - 1], bestc[NB - 1], accP, xn[NB - 1], cnP, codeP);

#pragma unroll
    for (int b = 0; b < NB; b++) {
        const long r = row0 + 32 * b + j;
        store_answer(bestd[b], cs::index_of(bestc[b], h), r, h == 0 && r < n, ids, dist);
    }
}

// ---------------------------------------------------------------------------------------------
// Hinted sweep (Lloyd iterations after the first).  Every row arrives with a guess -- its
// assignment in the previous iteration -- and rows are visited in an order that groups equal
// guesses (the member-list order the centroid update has just built).  The guess's distance is
// evaluated exactly up front (the same ascending fmaf chain, on the VALU) and becomes the running
// best, so during the sweep an accumulator can matter only if its minimum reaches that best:
// per accumulator the wave computes 16 unclamped distances and their minimum (2.5 VALU per
// element instead of 6) and enters the exact update -- lexicographic (distance, index), so that the
// answer is the brute-force arg-min with lowest-index ties whatever the guess was -- only when some
// lane needs it.  With grouped guesses that is the guess's own tile plus the rows that really move.
template <int D, int NB, int NA>
__global__ void __launch_bounds__(WG, 2)
assign_mfma_hinted_kernel(const float* __restrict__ X, long n, const float* __restrict__ C, int k,
                          const float* __restrict__ img, int ntiles, const uint32_t* __restrict__ order,
                          const long* __restrict__ hint, const uint32_t* __restrict__ hint_sorted,
                          long* __restrict__ ids, float* __restrict__ dist) {
    constexpr int R = tile_rows(NA);
    constexpr int TILE_F = tile_floats(D, NA);
    constexpr int PIECES = TILE_F / 256;
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 2 * TILE_F floats

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31;
    const int h = lane >> 5;
    const long pos0 = ((long)blockIdx.x * 4 + wave) * (32 * NB);

    float xr[NB][D / 2];
    float xn[NB];
    float bestd[NB];
    unsigned besti[NB];
    long rowid[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        long pos = pos0 + 32 * b + j;
        if (pos >= n) pos = n - 1;
        const long r = order ? (long)order[pos] : pos;
        rowid[b] = r;
        const f32x4* p = reinterpret_cast<const f32x4*>(X + r * D);
        // guesses listed in visiting order are one coalesced read; per-row guesses are a gather
        const long g = hint_sorted ? (long)hint_sorted[pos] : (hint ? hint[r] : -1);
        const bool has = g >= 0 && g < k;
        const f32x4* pc = reinterpret_cast<const f32x4*>(C + (has ? g : 0) * D);
        float nrm = 0.0f, cnn = 0.0f, ip = 0.0f;
        // exact distance to the guess: three ascending fmaf chains (rolled loop: keeps the register
        // footprint of this one-off prologue small)
#pragma clang loop unroll(disable)
        for (int q = 0; q < D / 4; q++) {
            const f32x4 u = p[q], cu = pc[q];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                nrm = __builtin_fmaf(u[e], u[e], nrm);
                cnn = __builtin_fmaf(cu[e], cu[e], cnn);
                ip = __builtin_fmaf(cu[e], u[e], ip);
            }
        }
        load_x_row<D>(X + r * D, h, xr[b]);
        xn[b] = nrm;
        const float dh = __builtin_fmaxf(__builtin_fmaf(-2.0f, ip, nrm + cnn), 0.0f);
        bestd[b] = has ? dh : __builtin_inff();
        besti[b] = has ? (unsigned)g : 0xffffffffu;
    }

    auto stage_tile = [&](int tile, float* dst) {
        const float* src = img + (size_t)tile * TILE_F;
#pragma unroll
        for (int p0 = 0; p0 < PIECES; p0 += 4) {
            const int p = p0 + wave;
            if (p < PIECES) dma_1k(src + p * 256 + lane * 4, dst + p * 256);
        }
    };
    stage_tile(0, smem);
    __syncthreads();

    for (int ct = 0; ct < ntiles; ct++) {
        const float* cur = smem + (ct & 1) * TILE_F;
        if (ct + 1 < ntiles) stage_tile(ct + 1, smem + ((ct + 1) & 1) * TILE_F);
#pragma unroll
        for (int a = 0; a < NA; a++) {
            f32x4 cnv[4];
            load_norms16(cur + R * D + a * 32 + 4 * h, cnv);
            const SwizzledRow arow{cur + (a * 32 + j) * D, j, h};
            const unsigned jobbase = (unsigned)cs::acc_base(ct * NA + a, h);
#pragma unroll
            for (int b = 0; b < NB; b++) {
                f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < D / 8; q++) mfma_fragment(acc, arow, q, xr[b]);
                // (written out, not lex_update16 with an index functor: in a helper the sixteen indices, the same for
                // every b, are lifted out of the row-block loop and <64, 2, 4> grows from 162 to 183 registers)
                if (__builtin_amdgcn_ballot_w64(min16_unclamped(acc, xn[b], cnv) <= bestd[b]) != 0) {
                    float bd = bestd[b];
                    unsigned bi = besti[b];
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const float dd = __builtin_fmaxf(dist_unclamped(acc, r, xn[b], cnv), 0.0f);
                        const unsigned idx = jobbase + (unsigned)cs::reg_offset(r);
                        const bool better = lex_better(dd, idx, bd, bi);
                        bd = better ? dd : bd;
                        bi = better ? idx : bi;
                    }
                    bestd[b] = bd;
                    besti[b] = bi;
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int b = 0; b < NB; b++) store_answer(bestd[b], besti[b], rowid[b], h == 0 && pos0 + 32 * b + j < n, ids, dist);
}

// ---------------------------------------------------------------------------------------------
// Pruned sweep (Lloyd iterations after the first; see prune.hip for the bound).  Same structure as
// the hinted sweep, but (1) the centroid image is in spatially grouped order (a table in the tile's
// pad maps image rows back to centroid indices for the lexicographic update), (2) every 32-row tile
// comes with a bit mask over the 32-centroid groups: an accumulator whose bit is clear is not
// computed at all, and a 128-centroid tile that no wave of the workgroup needs is not even staged.
// The running best starts from the exact distance to the guess (computed by the pre-pass).
__global__ void __launch_bounds__(WG) prep_centroids_perm_kernel(const float* __restrict__ c, int k, int d,
                                                                 const int32_t* __restrict__ cperm, int kp,
                                                                 int na, float* __restrict__ img) {
    const int t = blockIdx.x;
    const int R = tile_rows(na);
    float* out = img + (size_t)t * tile_floats(d, na);
    const int chunks_per_row = d / 4;
    for (int e = threadIdx.x; e < R * chunks_per_row; e += WG) {
        const int r = e / chunks_per_row, pc = e % chunks_per_row;
        const int slot = t * R + r;
        const int row = slot < kp ? cperm[slot] : -1;
        *reinterpret_cast<f32x4*>(out + (size_t)r * d + pc * 4) =
            image_slot(row >= 0 ? c + (size_t)row * d : nullptr, d, 0, r, pc);
    }
    for (int r = threadIdx.x; r < 128; r += WG) {
        const int slot = t * R + r;
        const int row = (r < R && slot < kp) ? cperm[slot] : -1;
        out[R * d + r] = image_norm(row >= 0 ? c + (size_t)row * d : nullptr, d);
        reinterpret_cast<unsigned*>(out)[R * d + 128 + r] = row >= 0 ? (unsigned)row : 0xffffffffu;
    }
}

// One wavefront per workgroup: a wave walks only the groups its own 32*NB rows need, staging one
// 32-centroid group (8 or 16 KiB + norms + index table) at a time through its private double buffer.
// No workgroup barrier anywhere: the LDS-DMA is issued and awaited (s_waitcnt vmcnt(0)) by the same
// wave that reads it.
constexpr int GROUP_PAD = 256;  // floats behind a group's rows: |c|^2 at [0,32), indices at [128,160)

template <int D, int NB>
__global__ void __launch_bounds__(64)
assign_mfma_pruned_kernel(const float* __restrict__ X, long n, const float* __restrict__ img, int ng,
                          const uint32_t* __restrict__ order, const uint32_t* __restrict__ hint_sorted,
                          const float* __restrict__ bd_in, const uint32_t* __restrict__ mask, int ngw,
                          long* __restrict__ ids, float* __restrict__ dist) {
    constexpr int GROUP_F = 32 * D + GROUP_PAD;
    constexpr int PIECES = GROUP_F / 256;
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 2 * GROUP_F floats

    const int lane = threadIdx.x;
    const int j = lane & 31;
    const int h = lane >> 5;
    const long pos0 = (long)blockIdx.x * (32 * NB);

    PrunedRows<D, NB> rows(X, n, order, hint_sorted, bd_in, mask, ng, ngw, pos0, j, h);
    auto stage_group = [&](int g, float* dst) {
        const float* src = img + (size_t)g * GROUP_F;
#pragma unroll
        for (int p = 0; p < PIECES; p++) dma_1k(src + p * 256 + lane * 4, dst + p * 256);
    };

    int g = rows.next_group(0);
    int buf = 0;
    if (g < ng) stage_group(g, smem);
    while (g < ng) {
        const float* cur = smem + buf * GROUP_F;
        // the group being consumed has landed once every DMA this wave issued so far is done; the
        // reads of the other buffer (previous group) were all consumed by that group's MFMAs
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int nxt = rows.next_group(g + 1);
        if (nxt < ng) stage_group(nxt, smem + (buf ^ 1) * GROUP_F);

        f32x4 cnv[4];
        load_norms16(cur + 32 * D + 4 * h, cnv);
        const SwizzledRow arow{cur + j * D, j, h};
        const unsigned* idxrow = reinterpret_cast<const unsigned*>(cur) + 32 * D + 128 + 4 * h;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            if (!rows.needs(b, g)) continue;
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < D / 8; q++) mfma_fragment(acc, arow, q, rows.xr[b]);
            lex_update16(rows.bestd[b], rows.besti[b], acc, rows.xn[b], cnv, idxrow);
        }
        g = nxt;
        buf ^= 1;
    }

#pragma unroll
    for (int b = 0; b < NB; b++)
        store_answer(rows.bestd[b], rows.besti[b], rows.rowid[b], h == 0 && pos0 + 32 * b + j < n, ids, dist);
}

// Register-staged form of the pruned sweep: the A fragments of the NEXT needed group are loaded
// from the (L2-resident) image straight into registers while the current group's MFMAs run, so
// there is no LDS, no DMA wait and no barrier at all; two register sets alternate (the loop body is
// written out for both roles).
template <int D, int NB>
__global__ void __launch_bounds__(64, 2)
assign_mfma_pruned_reg_kernel(const float* __restrict__ X, long n, const float* __restrict__ img, int ng,
                              const uint32_t* __restrict__ order, const uint32_t* __restrict__ hint_sorted,
                              const float* __restrict__ bd_in, const uint32_t* __restrict__ mask, int ngw,
                              long* __restrict__ ids, float* __restrict__ dist) {
    constexpr int GROUP_F = 32 * D + GROUP_PAD;
    constexpr int NQ = D / 8;

    const int lane = threadIdx.x;
    const int j = lane & 31;
    const int h = lane >> 5;
    const long pos0 = (long)blockIdx.x * (32 * NB);

    PrunedRows<D, NB> rows(X, n, order, hint_sorted, bd_in, mask, ng, ngw, pos0, j, h);

    auto load_group = [&](int g, f32x4 (&av)[NQ], f32x4 (&cn)[4]) {
        const float* base = img + (size_t)g * GROUP_F;
        const SwizzledRow arow{base + j * D, j, h};
#pragma unroll
        for (int q = 0; q < NQ; q++) av[q] = arow(q);
        load_norms16(base + 32 * D + 4 * h, cn);
    };
    auto compute_group = [&](int g, const f32x4 (&av)[NQ], const f32x4 (&cnv)[4]) {
        const unsigned* idxrow = reinterpret_cast<const unsigned*>(img + (size_t)g * GROUP_F) + 32 * D + 128 + 4 * h;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            if (!rows.needs(b, g)) continue;
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < NQ; q++) mfma_fragment(acc, RegRow<NQ>{av}, q, rows.xr[b]);
            lex_update16(rows.bestd[b], rows.besti[b], acc, rows.xn[b], cnv, idxrow);
        }
    };

    f32x4 avA[NQ], cnA[4], avB[NQ], cnB[4];
    int g = rows.next_group(0);
    if (g < ng) load_group(g, avA, cnA);
    while (g < ng) {
        const int g1 = rows.next_group(g + 1);
        if (g1 < ng) load_group(g1, avB, cnB);
        compute_group(g, avA, cnA);
        if (g1 >= ng) break;
        const int g2 = rows.next_group(g1 + 1);
        if (g2 < ng) load_group(g2, avA, cnA);
        compute_group(g1, avB, cnB);
        g = g2;
    }

#pragma unroll
    for (int b = 0; b < NB; b++)
        store_answer(rows.bestd[b], rows.besti[b], rows.rowid[b], h == 0 && pos0 + 32 * b + j < n, ids, dist);
}

// ---------------------------------------------------------------------------------------------
// Any d that is a multiple of 4 (n_mels other than 64/128, use_convolution's d = 10*n_mels):
// the same MFMA sweep with the feature axis cut into chunks of 64.  The NA*NB accumulators of a
// centroid tile stay live across the chunks (so every inner product is still ONE ascending fmaf
// chain); the centroid image is laid out [tile][chunk][row][64 swizzled] and streamed through LDS
// one (tile, chunk) piece at a time; the x chunk of a wave's rows is re-read from L2 per piece.
// The layout is chunked_sweep.h's, shared with the sweeps of knn.hip, ip.hip and rq.hip.
__global__ void __launch_bounds__(WG) prep_centroids_chunked_kernel(const float* __restrict__ c, int k,
                                                                    int d, int nchunks, int na,
                                                                    float* __restrict__ img) {
    const int t = blockIdx.x;
    const int R = tile_rows(na);
    float* out = img + (size_t)t * cs::tile_floats(na, nchunks);
    const int chunks16 = DC / 4;  // 16-byte slots per row piece
    for (int e = threadIdx.x; e < nchunks * R * chunks16; e += WG) {
        const int ch = e / (R * chunks16);
        const int r = (e / chunks16) % R, pc = e % chunks16;
        const int row = t * R + r;
        *reinterpret_cast<f32x4*>(out + ((size_t)ch * R + r) * DC + pc * 4) =
            image_slot(row < k ? c + (size_t)row * d : nullptr, d, ch * DC, r, pc);
    }
    for (int r = threadIdx.x; r < CN_PAD; r += WG) {
        const int row = t * R + r;
        out[(size_t)cs::piece_floats(na) * nchunks + r] = image_norm(r < R && row < k ? c + (size_t)row * d : nullptr, d);
    }
}

template <int NB, int NA, int WPS>
__global__ void __launch_bounds__(WG, WPS)
assign_mfma_anyd_kernel(const float* __restrict__ X, long n, int d, int nchunks,
                        const float* __restrict__ img, int ntiles, long* __restrict__ ids,
                        float* __restrict__ dist) {
    constexpr int PIECE_F = cs::piece_floats(NA);   // floats of one (tile, chunk) piece
    constexpr int BUF_F = cs::buf_floats(NA);       // + the norms behind the last chunk
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 2 * BUF_F floats

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31;
    const int h = lane >> 5;
    const long row0 = ((long)blockIdx.x * 4 + wave) * (32 * NB);
    const size_t tile_f = cs::tile_floats(NA, nchunks);

    const float* xrow[NB];
    float xn[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        long r = row0 + 32 * b + j;
        if (r >= n) r = n - 1;
        xrow[b] = X + r * d;
        xn[b] = cs::sqnorm16(xrow[b], d);
    }

    float bestd[NB];
    unsigned bestc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        bestd[b] = __builtin_inff();
        bestc[b] = 0xffffffffu;
    }

    // piece s = ct * nchunks + ch lives at img + ct*tile_f + ch*PIECE_F; the last chunk drags the
    // norms along (they sit right behind it), so the count of 1 KiB pieces is known only here
    auto stage_piece = [&](int ct, int ch, float* dst) {
        const float* src = img + (size_t)ct * tile_f + (size_t)ch * PIECE_F;
        const int pieces = (ch == nchunks - 1 ? BUF_F : PIECE_F) / 256;
        for (int p = wave; p < pieces; p += 4) dma_1k(src + p * 256 + lane * 4, dst + p * 256);
    };
    stage_piece(0, 0, smem);
    __syncthreads();

    const int nstages = ntiles * nchunks;
    int ct = 0, ch = 0;
    f32x16 acc[NA][NB];
    // A wave's x chunk (features chx*64 .. +63 of its 32*NB rows, zero past d) as the B operand.  Two register
    // sets alternate: the chunk of stage s+1 is requested from L2 before the MFMAs of stage s are issued, so its
    // latency runs beside them instead of in front of the next stage (round 1 reloaded it at the top of every stage
    // and waited: 41-55 % of the fp32 MFMA peak at d = 640).
    auto load_x = [&](int chx, float (&xr)[NB][DC / 2]) {
#pragma unroll
        for (int b = 0; b < NB; b++) cs::load_x_chunk(xrow[b], chx, d, h, xr[b]);
    };
    auto stage = [&](int s, const float (&xr)[NB][DC / 2], float (&xr_next)[NB][DC / 2]) {
        const float* cur = smem + (s & 1) * BUF_F;
        {
            int nct = ct, nch = ch + 1;
            if (nch == nchunks) { nch = 0; nct++; }
            if (s + 1 < nstages) {
                stage_piece(nct, nch, smem + ((s + 1) & 1) * BUF_F);
                load_x(nch, xr_next);
            }
        }
#pragma unroll
        for (int a = 0; a < NA; a++) {
            const SwizzledRow arow{cur + (a * 32 + j) * DC, j, h};
#pragma unroll
            for (int b = 0; b < NB; b++) {
                f32x16 cacc = acc[a][b];
                if (ch == 0) cacc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < DC / 8; q++) mfma_fragment(cacc, arow, q, xr[b]);
                acc[a][b] = cacc;
            }
        }
        if (ch == nchunks - 1) {  // tile finished: arg-min over its NA*NB accumulators
#pragma unroll
            for (int a = 0; a < NA; a++) {
                f32x4 cnv[4];
                load_norms16(cur + PIECE_F + a * 32 + 4 * h, cnv);
                const unsigned codebase = (unsigned)(ct * NA + a) * 16u;
#pragma unroll
                for (int b = 0; b < NB; b++) epilogue16(bestd[b], bestc[b], acc[a][b], xn[b], cnv, codebase);
            }
        }
        if (++ch == nchunks) { ch = 0; ct++; }
        __syncthreads();
    };
    float xrA[NB][DC / 2], xrB[NB][DC / 2];
    load_x(0, xrA);
    for (int s = 0; s < nstages; s += 2) {
        stage(s, xrA, xrB);
        if (s + 1 < nstages) stage(s + 1, xrB, xrA);
    }

#pragma unroll
    for (int b = 0; b < NB; b++) {
        const long r = row0 + 32 * b + j;
        store_answer(bestd[b], cs::index_of(bestc[b], h), r, h == 0 && r < n, ids, dist);
    }
}

// ---------------------------------------------------------------------------------------------
// Any d at all (fallback: scalar fmaf chains, one thread per row; same arithmetic as the MFMA path).
// Used only when d is not a multiple of 4 or the rows are not 16-byte aligned.
__global__ void __launch_bounds__(WG)
assign_generic_kernel(const float* __restrict__ X, long n, int d, const float* __restrict__ C,
                      const float* __restrict__ cn, int k, long* __restrict__ ids,
                      float* __restrict__ dist) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const float* xi = X + i * d;
    float xn = 0.0f;
    for (int f = 0; f < d; f++) xn = __builtin_fmaf(xi[f], xi[f], xn);
    float best = __builtin_inff();
    long bi = -1;
    for (int c = 0; c < k; c++) {
        const float* cc = C + (size_t)c * d;
        float ip = 0.0f;
        for (int f = 0; f < d; f++) ip = __builtin_fmaf(xi[f], cc[f], ip);
        float dis = __builtin_fmaf(-2.0f, ip, xn + cn[c]);
        dis = __builtin_fmaxf(dis, 0.0f);
        if (dis < best) {
            best = dis;
            bi = c;
        }
    }
    ids[i] = bi;
    if (dist) dist[i] = best;
}

__global__ void __launch_bounds__(WG) row_sqnorm_kernel(const float* __restrict__ C, int k, int d,
                                                        float* __restrict__ cn) {
    const int c = blockIdx.x * WG + threadIdx.x;
    if (c >= k) return;
    float s = 0.0f;
    for (int f = 0; f < d; f++) s = __builtin_fmaf(C[(size_t)c * d + f], C[(size_t)c * d + f], s);
    cn[c] = s;
}

// faiss exhaustive_L2sqr_seq (n < distance_compute_blas_threshold = 20): direct sum (x-c)^2.
__global__ void assign_small_kernel(const float* __restrict__ X, int n, int d,
                                    const float* __restrict__ C, int k, long* __restrict__ ids,
                                    float* __restrict__ dist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float best = __builtin_inff();
    long bi = -1;
    for (int c = 0; c < k; c++) {
        float acc = 0.0f;
        for (int f = 0; f < d; f++) {
            const float df = X[(size_t)i * d + f] - C[(size_t)c * d + f];
            acc = __builtin_fmaf(df, df, acc);
        }
        if (acc < best) {
            best = acc;
            bi = c;
        }
    }
    ids[i] = bi;
    if (dist) dist[i] = best;
}

// the tiled centroid image of the dense and the hinted sweeps (tiles of 32 * na rows) in WS_CENT_IMG
int prep_image(at_ctx* ctx, const float* c, int k, int d, int na, hipStream_t stream, float** img_out, int* ntiles_out) {
    const int ntiles = (k + tile_rows(na) - 1) / tile_rows(na);
    float* img = static_cast<float*>(at_ws(ctx, WS_CENT_IMG, sizeof(float) * (size_t)ntiles * tile_floats(d, na), stream));
    if (!img) return AT_E_NOMEM;
    AT_LAUNCH(prep_centroids_kernel, dim3(ntiles), dim3(WG), 0, stream, c, k, d, d, na, img);
    *img_out = img;
    *ntiles_out = ntiles;
    return AT_OK;
}

template <int D, int NB, int NA, bool DMA, int WPS, bool SPEC = false>
int launch_mfma(at_ctx* ctx, const float* x, int64_t n, const float* c, int k, int64_t* ids, float* dist,
                hipStream_t stream) {
    int ntiles = 0;
    float* img = nullptr;
    const int rc = prep_image(ctx, c, k, D, NA, stream, &img, &ntiles);
    if (rc) return rc;
    const size_t lds = 2 * sizeof(float) * tile_floats(D, NA);
    const int64_t rows_per_wg = 4 * 32 * NB;
    const int64_t grid = (n + rows_per_wg - 1) / rows_per_wg;
    AT_RAISE_LDS(ctx, (assign_mfma_kernel<D, NB, NA, DMA, WPS, SPEC>), lds);
    AT_LAUNCH((assign_mfma_kernel<D, NB, NA, DMA, WPS, SPEC>), dim3((unsigned)grid), dim3(WG), lds,
                       stream, x, (long)n, img, ntiles, reinterpret_cast<long*>(ids), dist);
    return AT_OK;
}


template <int NB, int NA, int WPS>
static int launch_anyd(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k, int64_t* ids, float* dist,
                       hipStream_t stream) {
    const int nchunks = cs::nchunks_of(d);
    const int ntiles = (k + tile_rows(NA) - 1) / tile_rows(NA);
    const size_t tile_f = cs::tile_floats(NA, nchunks);
    float* img = static_cast<float*>(at_ws(ctx, WS_CENT_IMG, sizeof(float) * ntiles * tile_f, stream));
    if (!img) return AT_E_NOMEM;
    AT_LAUNCH(prep_centroids_chunked_kernel, dim3(ntiles), dim3(WG), 0, stream, c, k, d, nchunks, NA, img);
    const size_t lds = 2 * sizeof(float) * cs::buf_floats(NA);
    AT_RAISE_LDS(ctx, (assign_mfma_anyd_kernel<NB, NA, WPS>), lds);
    const int64_t rows_per_wg = 4 * 32 * NB;
    AT_LAUNCH((assign_mfma_anyd_kernel<NB, NA, WPS>), dim3((unsigned)((n + rows_per_wg - 1) / rows_per_wg)),
                       dim3(WG), lds, stream, x, (long)n, d, nchunks, img, ntiles, reinterpret_cast<long*>(ids), dist);
    return AT_OK;
}

}  // namespace

int at_prep_chunked_image(at_ctx* ctx, const float* c, int k, int d, int na, float* img, hipStream_t stream) {
    (void)ctx;
    const int ntiles = (k + tile_rows(na) - 1) / tile_rows(na);
    AT_LAUNCH(prep_centroids_chunked_kernel, dim3(ntiles), dim3(WG), 0, stream, c, k, d, cs::nchunks_of(d), na, img);
    return AT_OK;
}

extern "C" int at_assign_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k,
                             int64_t* ids, float* dist, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx, "at_assign_f32: ctx is null");
    AT_REQUIRE(n >= 0 && d > 0 && k > 0, "at_assign_f32: bad sizes n=%lld d=%d k=%d", (long long)n, d, k);
    if (n == 0) return AT_OK;
    AT_REQUIRE(x && c && ids, "at_assign_f32: null pointer");
    AT_REQUIRE(k <= (1 << 24), "at_assign_f32: k=%d too large", k);
    AT_HIP(hipSetDevice(ctx->device));

    if (n < 20) {
        AT_LAUNCH(assign_small_kernel, dim3(1), dim3(32), 0, stream, x, (int)n, d, c, k,
                           reinterpret_cast<long*>(ids), dist);
        return AT_OK;
    }

    if (d == 64 || d == 128) {
        AT_REQUIRE(at_aligned16(x), "at_assign_f32: x must be 16-byte aligned");
        // Shipped shapes: LDS-DMA staging, 128-centroid tiles at d=64 (64 at d=128), 2 waves/SIMD.
        // AT_ASSIGN_VARIANT=1 selects the register-staged 64-centroid-tile kernel (A/B aid).
        const int v = ctx->dbg.assign_variant;
        if (d == 64) {
            if (v == 1) return launch_mfma<64, 2, 2, false, 2>(ctx, x, n, c, k, ids, dist, stream);
            if (v == 3) return launch_mfma<64, 2, 4, true, 2, true>(ctx, x, n, c, k, ids, dist, stream);
            return launch_mfma<64, 2, 4, true, 2>(ctx, x, n, c, k, ids, dist, stream);
        }
        if (v == 1) return launch_mfma<128, 1, 2, false, 2>(ctx, x, n, c, k, ids, dist, stream);
        if (v == 3) return launch_mfma<128, 1, 2, true, 2, true>(ctx, x, n, c, k, ids, dist, stream);
        return launch_mfma<128, 1, 2, true, 2>(ctx, x, n, c, k, ids, dist, stream);
    }

    if (d % 4 == 0 && at_aligned16(x) && ctx->dbg.assign_variant != 2) {
        // shapes (assign_variant: A/B aid): 0 = two row tiles x two centroid tiles per wave at one wave per SIMD (both
        // x-chunk register sets fit); 4 = one row tile at two waves per SIMD
        const int v = ctx->dbg.assign_variant;
        if (v == 4) return launch_anyd<1, 2, 2>(ctx, x, n, d, c, k, ids, dist, stream);
        if (v == 5) return launch_anyd<1, 2, 3>(ctx, x, n, d, c, k, ids, dist, stream);
        if (v == 6) return launch_anyd<2, 2, 1>(ctx, x, n, d, c, k, ids, dist, stream);
        return launch_anyd<1, 4, 2>(ctx, x, n, d, c, k, ids, dist, stream);
    }

    float* cn = static_cast<float*>(at_ws(ctx, WS_CENT_IMG, sizeof(float) * (size_t)k, stream));
    if (!cn) return AT_E_NOMEM;
    AT_LAUNCH(row_sqnorm_kernel, dim3((k + WG - 1) / WG), dim3(WG), 0, stream, c, k, d, cn);
    AT_LAUNCH(assign_generic_kernel, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0,
                       stream, x, (long)n, d, c, cn, k, reinterpret_cast<long*>(ids), dist);
    return AT_OK;
}

// The hinted sweep of one shape (the two shipped: d = 64 and d = 128).
template <int D, int NB, int NA>
static int launch_hinted(at_ctx* ctx, const float* x, int64_t n, const float* c, int k, const int64_t* hint_ids,
                         const uint32_t* order, const uint32_t* hint_sorted, int64_t* ids, float* dist, hipStream_t stream) {
    int ntiles = 0;
    float* img = nullptr;
    const int rc = prep_image(ctx, c, k, D, NA, stream, &img, &ntiles);
    if (rc) return rc;
    const size_t lds = 2 * sizeof(float) * tile_floats(D, NA);
    AT_RAISE_LDS(ctx, (assign_mfma_hinted_kernel<D, NB, NA>), lds);
    const int64_t rows_per_wg = 4 * 32 * NB;
    AT_LAUNCH((assign_mfma_hinted_kernel<D, NB, NA>), dim3((unsigned)((n + rows_per_wg - 1) / rows_per_wg)),
                       dim3(WG), lds, stream, x, (long)n, c, k, img, ntiles, order,
                       reinterpret_cast<const long*>(hint_ids), hint_sorted, reinterpret_cast<long*>(ids), dist);
    return AT_OK;
}

extern "C" int at_assign_hinted_f32(at_ctx* ctx, const float* x, int64_t n, int d, const float* c, int k,
                                    const int64_t* hint_ids, const uint32_t* order,
                                    const uint32_t* hint_sorted, int64_t* ids, float* dist, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx, "at_assign_hinted_f32: ctx is null");
    // shapes without a hinted kernel, or no hints at all: the plain sweep gives the same answer
    if (hint_sorted && !order) hint_sorted = nullptr;  // positions mean nothing without the order
    if ((!hint_ids && !hint_sorted) || n < 20 || !(d == 64 || d == 128) || !at_aligned16(x) || !at_aligned16(c))
        return at_assign_f32(ctx, x, n, d, c, k, ids, dist, stream_);
    AT_REQUIRE(n >= 0 && k > 0 && k <= (1 << 24) && n < (int64_t)UINT32_MAX, "at_assign_hinted_f32: bad sizes");
    AT_REQUIRE(x && c && ids, "at_assign_hinted_f32: null pointer");
    AT_REQUIRE(ids != hint_ids, "at_assign_hinted_f32: ids must not alias hint_ids");
    AT_HIP(hipSetDevice(ctx->device));
    if (d == 64) return launch_hinted<64, 2, 4>(ctx, x, n, c, k, hint_ids, order, hint_sorted, ids, dist, stream);
    return launch_hinted<128, 1, 2>(ctx, x, n, c, k, hint_ids, order, hint_sorted, ids, dist, stream);
}

// ---- the two launches of the exact pruned search that live here (driver: exact_search.cpp) --------------------
// fp32 image (one tile per group, NA = 1: 32 rows, then |c|^2 at [0,32) and indices at [128,160)): every call claims
// WS_CENT_IMG for it first, into call.img; it is built only where the fp32 sweep runs
int at_pruned_image_claim(at_ctx* ctx, at_exact_call& call) {
    call.img = static_cast<float*>(at_ws(ctx, WS_CENT_IMG, sizeof(float) * (size_t)call.ng * tile_floats(call.d, 1), call.stream));
    return call.img ? AT_OK : AT_E_NOMEM;
}

int at_pruned_image_build(at_ctx* ctx, const at_exact_call& call) {
    (void)ctx;
    AT_LAUNCH(prep_centroids_perm_kernel, dim3(call.ng), dim3(WG), 0, call.stream, call.c, call.k, call.d, call.cperm,
              call.ng * 32, 1, call.img);
    return AT_OK;
}

template <int D, int NB>
static int launch_pruned_sweep(at_ctx* ctx, const at_exact_call& call, int64_t n, const uint32_t* order,
                               const uint32_t* hint_sorted) {
    const size_t lds = 2 * sizeof(float) * tile_floats(D, 1);
    const int64_t rows_per_wg = 32 * NB;
    // d = 64, one or two row tiles: register-staged A operand (no LDS); AT_PRUNE_KERNEL=0 selects the LDS-DMA form
    // (A/B aid).  Every other shape has the LDS-DMA form only, so the register form is not even instantiated there.
    if constexpr (D == 64 && NB <= 2) {
        if (ctx->dbg.prune_kernel != 0) {
            AT_LAUNCH((assign_mfma_pruned_reg_kernel<D, NB>), dim3((unsigned)((n + rows_per_wg - 1) / rows_per_wg)),
                               dim3(64), 0, call.stream, call.x, (long)n, call.img, call.ng, order, hint_sorted, call.bd, call.mask,
                               call.ngw, reinterpret_cast<long*>(call.ids), call.dist);
            return AT_OK;
        }
    }
    AT_LAUNCH((assign_mfma_pruned_kernel<D, NB>), dim3((unsigned)((n + rows_per_wg - 1) / rows_per_wg)),
                       dim3(64), lds, call.stream, call.x, (long)n, call.img, call.ng, order, hint_sorted, call.bd, call.mask,
                       call.ngw, reinterpret_cast<long*>(call.ids), call.dist);
    return AT_OK;
}

int at_pruned_sweep_f32(at_ctx* ctx, const at_exact_call& call, int64_t n, const uint32_t* order, const uint32_t* hint_sorted) {
    if (call.d == 64) {
        const int nbsw = ctx->dbg.prune_nb;
        if (nbsw == 4) return launch_pruned_sweep<64, 4>(ctx, call, n, order, hint_sorted);
        if (nbsw == 1) return launch_pruned_sweep<64, 1>(ctx, call, n, order, hint_sorted);
        return launch_pruned_sweep<64, 2>(ctx, call, n, order, hint_sorted);
    }
    return launch_pruned_sweep<128, 2>(ctx, call, n, order, hint_sorted);
}
