// prune.hip -- the bookkeeping that lets a Lloyd iteration skip most of the -2XC^T work without
// changing a single output bit (used by at_assign_pruned_f32, exact_search.cpp).
//
// Replaces nothing in the reference by itself: it accelerates the search inside
// faiss.Kmeans.train (processors/cluster_creator.py:54-56 of danavery/audio-tokens) from the second
// Lloyd iteration on.
//
// Idea (Elkan's lemma, made safe for fp32): row x was assigned to centroid p in the previous
// iteration; its distance to the UPDATED c_p is evaluated exactly (same fmaf chains as the MFMA
// sweep) and is an upper bound bd of its final minimum.  For any other centroid c,
// |x - c| >= |c - c_p| - |x - c_p|, so c cannot reach bd when |c - c_p| > 2 |x - c_p|.  To be
// certain about the COMPUTED distances, which differ from the true ones by at most
// delta = (2d + 8) u (|x|^2 + max|c|^2), the radius is inflated: R = sqrt(bd + delta), skip iff
// (a lower bound of) |c - c_p| > 2 R.  Centroids are handled in groups of 32 (one MFMA
// accumulator) laid out by a kd-style spatial grouping, rows in tiles of 32 visited in
// (previous centroid, distance) order so that the outliers of a cluster sit together.
// At the ends of the fp32 range the real-number argument needs two guards (tests/test_gpu_magnitude.py):
// the direct sum |c - c_p|^2 overflows from |c - c_p| ~ 1.84e19 although the sweep's (xn + cn) - 2 ip
// is finite for rows between the two, so a sum that is not finite bounds nothing (dmin = 0); and a radius
// that comes out NaN (a non-finite row, a NaN centroid norm) compares false with every dmin, so it is read
// as +inf.  A row with |x|^2 = +inf has delta = +inf and visits every group; it ends as (-1, +inf)
// (assign.hip, no_winner).  Subnormal sums need nothing: delta's relative model is a handful of
// subnormal ulps there, but the bound kernel's 2e-5 and the sqrt absorb the absolute half-ulp per step
// (measured: the 2^-64 rung prunes like the unit one and keeps every bit).
//   group_min_dist_kernel : dmin[p][g] = lower bound of min_{c in group g} |c - c_p|
//   visit order           : stable radix sort of (p << 8 | quantised distance, row)
//   prune_mask_kernel     : per row bd; per 32-row tile one bit per group ("some row needs it")
#include <cstdlib>
#include <cstring>

#include "at_internal.h"
#include "at_sort.h"

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int WG = 256;
constexpr float U32 = 5.9604645e-8f;  // 2^-24

// ---- dmin[p][g] ------------------------------------------------------------------------------
// grid (ng, ceil(k/256)); the group's <= 32 rows sit in LDS (read as broadcasts); one thread per p
// with its own row in registers.
template <int D>
__global__ void __launch_bounds__(WG) group_min_dist_kernel(const float* __restrict__ C, int k,
                                                            const int32_t* __restrict__ cperm, int ng,
                                                            float* __restrict__ dmin) {
    __shared__ __attribute__((aligned(16))) float grp[32 * D];
    __shared__ int member[32];
    const int g = blockIdx.x;
    if (threadIdx.x < 32) member[threadIdx.x] = cperm[g * 32 + threadIdx.x];
    __syncthreads();
    for (int e = threadIdx.x; e < 32 * (D / 4); e += WG) {
        const int m = member[e / (D / 4)];
        f32x4_t v = {0, 0, 0, 0};
        if (m >= 0) v = reinterpret_cast<const f32x4_t*>(C + (size_t)m * D)[e % (D / 4)];
        reinterpret_cast<f32x4_t*>(grp)[e] = v;
    }
    __syncthreads();
    int p = blockIdx.y * WG + threadIdx.x;
    const bool livep = p < k;
    if (!livep) p = k - 1;
    f32x4_t cp[D / 4];
#pragma unroll
    for (int q = 0; q < D / 4; q++) cp[q] = reinterpret_cast<const f32x4_t*>(C + (size_t)p * D)[q];
    float best = __builtin_inff();
    for (int m = 0; m < 32; m++) {
        if (member[m] < 0) continue;  // uniform
        const f32x4_t* cg = reinterpret_cast<const f32x4_t*>(grp + m * D);
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int q = 0; q < D / 4; q++) {
            const f32x4_t b = cg[q];
            const float d0 = cp[q][0] - b[0], d1 = cp[q][1] - b[1], d2 = cp[q][2] - b[2], d3 = cp[q][3] - b[3];
            s0 = __builtin_fmaf(d0, d0, s0);
            s1 = __builtin_fmaf(d1, d1, s1);
            s0 = __builtin_fmaf(d2, d2, s0);
            s1 = __builtin_fmaf(d3, d3, s1);
        }
        // |c_p - c_m|^2 overflows from |c_p - c_m| ~ 1.84e19 while the sweep's (xn + cn) - 2 ip is still finite for rows
        // between the two: a sum that is not finite bounds nothing (0: the group is always visited)
        const float s = s0 + s1;
        best = fminf(best, s < __builtin_inff() ? s : 0.0f);
    }
    // the fp32 sum of squared fp32 differences is within (d+3)u of the true value: shave 2e-5
    if (livep) dmin[(size_t)p * ng + g] = best == __builtin_inff() ? best : sqrtf(best) * (1.0f - 2e-5f);
}

// ---- visiting order --------------------------------------------------------------------------
__global__ void __launch_bounds__(WG) visit_keys_kernel(const long* __restrict__ ids,
                                                        const float* __restrict__ dis, long n, int k,
                                                        uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals, int dbits) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const long c = ids[i];
    const bool ok = c >= 0 && c < k;
    const float top = (float)((1u << dbits) - 1u);
    float r = dis ? sqrtf(fmaxf(dis[i], 0.0f)) * (0.5f * top) : 0.0f;   // unit rows: r <= 2
    r = fminf(r, top);
    keys[i] = ((ok ? (uint32_t)c : (uint32_t)k) << dbits) | (uint32_t)r;
    vals[i] = (uint32_t)i;
}

// the sorted keys give the guesses in visiting order; the sorted values (row indices) leave the sort's buffer in the same pass.
//
// Block schedules (exact_plan.h): the filter sweep's cost per row block is the number of centroid groups its tiles must
// visit, and that grows with the Elkan radius of the tile's outermost row.  The sorted keys still hold the quantised
// distance, so the same pass writes a weight per 32-row tile (weight != null; a wave holds two tiles): its largest
// distance field, scaled to 0..255, or 255 outright where the need set is wide whatever the distances say -- a row
// without a guess (every group), or rows of two clusters (the union of two unrelated sets).  Integer only.
__global__ void __launch_bounds__(WG) key_to_hint_kernel(const uint32_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ vals, long n,
                                                         uint32_t* __restrict__ hint_sorted,
                                                         uint32_t* __restrict__ order_out, int dbits, int k,
                                                         unsigned char* __restrict__ weight) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (i - lane >= n) return;                              // (the whole wave)
    const uint32_t key = keys[i < n ? i : n - 1];           // (past the end: the last row again)
    if (i < n) {
        hint_sorted[i] = key >> dbits;
        order_out[i] = vals[i];
    }
    if (!weight) return;
    const uint32_t cluster = key >> dbits;
    const uint32_t field = key & ((1u << dbits) - 1u);
    int w = (int)(dbits >= 8 ? field >> (dbits - 8) : field << (8 - dbits));
    if (cluster >= (uint32_t)k) w = exact_plan::SCHED_WEIGHT_MAX;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) w = max(w, __shfl_xor(w, off));
    const int first = __shfl((int)cluster, lane & 32), last = __shfl((int)cluster, (lane & 32) + 31);
    if (first != last) w = exact_plan::SCHED_WEIGHT_MAX;
    if ((lane & 31) == 0 && i < n) weight[i / 32] = (unsigned char)w;
}

// The class of block b of `nb` tiles: the top bits of the largest weight among its tiles.
__device__ __forceinline__ int sched_block_class(const unsigned char* __restrict__ weight, long tiles, long b, int nb) {
    int w = 0;
    for (int t = 0; t < nb; t++)
        if (b * nb + t < tiles) w = max(w, (int)weight[b * nb + t]);
    return exact_plan::sched_class(w);
}

// Stable counting sort of the blocks by descending class, for the three block sizes at once (blockIdx.y: 1, 2, 4 tiles);
// a workgroup owns SCHED_CHUNK consecutive blocks, eight rounds of 256.
//   sched_hist_kernel    hist[size][chunk][class] = blocks of the class in the chunk
//   sched_scan_kernel    ... -> where the chunk's blocks of the class start in the table (one workgroup per size)
//   sched_scatter_kernel table[start + rank within the chunk] = block
__global__ void __launch_bounds__(WG) sched_hist_kernel(const unsigned char* __restrict__ weight, long tiles, long chunks,
                                                        uint32_t* __restrict__ hist) {
    constexpr int NC = exact_plan::SCHED_CLASSES;
    __shared__ unsigned cnt[NC];
    const int nb = 1 << blockIdx.y;
    const long blocks = (tiles + nb - 1) / nb;
    const long base = (long)blockIdx.x * exact_plan::SCHED_CHUNK;
    if (base >= blocks) return;
    if (threadIdx.x < NC) cnt[threadIdx.x] = 0u;
    __syncthreads();
    for (int r = 0; r < exact_plan::SCHED_CHUNK / WG; r++) {
        const long b = base + r * WG + threadIdx.x;
        if (b < blocks) atomicAdd(&cnt[sched_block_class(weight, tiles, b, nb)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < NC) hist[((size_t)blockIdx.y * chunks + blockIdx.x) * NC + threadIdx.x] = cnt[threadIdx.x];
}

// (the counts pass through LDS in pieces of SCAN_PIECE chunks, so that the serial part never waits for global memory:
// a Lloyd-sized order has 32 chunks, one piece)
constexpr int SCAN_PIECE = 128;
__global__ void __launch_bounds__(WG) sched_scan_kernel(long tiles, long chunks, uint32_t* __restrict__ hist) {
    constexpr int NC = exact_plan::SCHED_CLASSES;
    __shared__ unsigned piece[SCAN_PIECE * NC], run[NC], start[NC];
    const int nb = 1 << blockIdx.x;
    const long blocks = (tiles + nb - 1) / nb;
    const long used = (blocks + exact_plan::SCHED_CHUNK - 1) / exact_plan::SCHED_CHUNK;   // chunks of this block size
    uint32_t* h = hist + (size_t)blockIdx.x * chunks * NC;
    const int t = threadIdx.x;
    // pass 0: counts -> exclusive sums within the class, chunks ascending; then the classes, descending;
    // pass 1: + where the class starts
    for (int pass = 0; pass < 2; pass++) {
        if (t < NC) run[t] = 0u;
        for (long p0 = 0; p0 < used; p0 += SCAN_PIECE) {
            const int m = (int)min((long)SCAN_PIECE, used - p0) * NC;
            __syncthreads();
            for (int e = t; e < m; e += WG) piece[e] = h[p0 * NC + e];
            __syncthreads();
            if (t < NC) {
                if (pass == 0) {
                    unsigned r = run[t];
                    for (int e = t; e < m; e += NC) {
                        const unsigned v = piece[e];
                        piece[e] = r;
                        r += v;
                    }
                    run[t] = r;
                } else {
                    for (int e = t; e < m; e += NC) piece[e] += start[t];
                }
            }
            __syncthreads();
            for (int e = t; e < m; e += WG) h[p0 * NC + e] = piece[e];
        }
        __syncthreads();
        if (pass == 0 && t == 0) {
            unsigned r = 0;
            for (int q = NC - 1; q >= 0; q--) {
                start[q] = r;
                r += run[q];
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(WG) sched_scatter_kernel(const unsigned char* __restrict__ weight, long tiles, long chunks,
                                                           const uint32_t* __restrict__ hist, uint32_t* __restrict__ table0,
                                                           uint32_t* __restrict__ table1, uint32_t* __restrict__ table2) {
    constexpr int NC = exact_plan::SCHED_CLASSES;
    constexpr int NW = WG / 64;
    __shared__ unsigned next[NC], wave_cnt[NW][NC];
    const int nb = 1 << blockIdx.y;
    const long blocks = (tiles + nb - 1) / nb;
    const long base = (long)blockIdx.x * exact_plan::SCHED_CHUNK;
    if (base >= blocks) return;
    uint32_t* table = blockIdx.y == 0 ? table0 : blockIdx.y == 1 ? table1 : table2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < NC) next[threadIdx.x] = hist[((size_t)blockIdx.y * chunks + blockIdx.x) * NC + threadIdx.x];
    for (int r = 0; r < exact_plan::SCHED_CHUNK / WG; r++) {
        const long b = base + r * WG + threadIdx.x;
        const int cls = b < blocks ? sched_block_class(weight, tiles, b, nb) : -1;
        unsigned below = 0;   // blocks of my class on lower lanes of my wave
        for (int q = 0; q < NC; q++) {
            const unsigned long long m = __builtin_amdgcn_ballot_w64(cls == q);
            if (cls == q) below = (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
            if (lane == 0) wave_cnt[wave][q] = (unsigned)__builtin_popcountll(m);
        }
        __syncthreads();   // (also: next[] of the round before)
        if (cls >= 0) {
            unsigned at = next[cls] + below;
            for (int w = 0; w < wave; w++) at += wave_cnt[w][cls];
            if (at < (unsigned long)blocks) table[at] = (uint32_t)b;   // (always, by the histogram: no write past the table)
        }
        __syncthreads();
        if (threadIdx.x < NC)
            for (int w = 0; w < NW; w++) next[threadIdx.x] += wave_cnt[w][threadIdx.x];
        __syncthreads();   // (wave_cnt is rewritten by the next round)
    }
}

__global__ void __launch_bounds__(WG) max_sqnorm_kernel(const float* __restrict__ C, int k, int d,
                                                        unsigned* __restrict__ out_bits) {
    const int c = blockIdx.x * WG + threadIdx.x;
    float s = 0.0f;
    if (c < k)
        for (int f = 0; f < d; f++) s = __builtin_fmaf(C[(size_t)c * d + f], C[(size_t)c * d + f], s);
    // non-negative floats order like their bit patterns
    atomicMax(out_bits, __float_as_uint(s));
}

// ---- per-row bound and per-tile group mask ----------------------------------------------------
// One wave per 64 visiting positions (two 32-row tiles: lanes 0-31 and 32-63).
template <int D>
__global__ void __launch_bounds__(WG) prune_mask_kernel(const float* __restrict__ X, long n,
                                                        const float* __restrict__ C, int k,
                                                        const uint32_t* __restrict__ order,
                                                        const uint32_t* __restrict__ hint_sorted,
                                                        const float* __restrict__ dmin, int ng,
                                                        const unsigned* __restrict__ cnmax_bits,
                                                        float* __restrict__ bd_out,
                                                        uint32_t* __restrict__ mask, int ngw,
                                                        unsigned long long* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long wpos = ((long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6)) * 64;
    if (wpos >= n) return;
    long pos = wpos + lane;
    const bool live = pos < n;
    if (!live) pos = n - 1;
    const long r = order[pos];
    const uint32_t p = hint_sorted[pos];
    const bool has = p < (uint32_t)k;
    const f32x4_t* px = reinterpret_cast<const f32x4_t*>(X + r * D);
    const f32x4_t* pc = reinterpret_cast<const f32x4_t*>(C + (size_t)(has ? p : 0) * D);
    // every load of the two rows is issued before the first dependent fma: a row-per-lane read that
    // waits for each 16-byte piece in turn keeps its 128-byte lines alive for many microseconds, and
    // with 2048 waves doing so they fall out of L2 and are fetched again (2.4x the bytes, measured)
    f32x4_t xv[D / 4], cv[D / 4];
#pragma unroll
    for (int q = 0; q < D / 4; q++) xv[q] = px[q];
#pragma unroll
    for (int q = 0; q < D / 4; q++) cv[q] = pc[q];
    float xn = 0.0f, cn = 0.0f, ip = 0.0f;
#pragma unroll
    for (int q = 0; q < D / 4; q++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            xn = __builtin_fmaf(xv[q][e], xv[q][e], xn);
            cn = __builtin_fmaf(cv[q][e], cv[q][e], cn);
            ip = __builtin_fmaf(cv[q][e], xv[q][e], ip);
        }
    }
    // exactly the value the MFMA sweep would produce for (x, c_p)
    const float dh = __builtin_fmaxf(__builtin_fmaf(-2.0f, ip, xn + cn), 0.0f);
    if (live) bd_out[pos] = has ? dh : __builtin_inff();

    const float cnmax = __uint_as_float(*cnmax_bits);
    const float delta = (2.0f * D + 8.0f) * U32 * (xn + cnmax) * 1.01f;
    // rows without a guess need every group; positions past n need none
    float tau = has ? 2.0f * sqrtf(dh + delta) * (1.0f + 4.0f * U32) + 1e-30f : __builtin_inff();
    if (!(tau == tau)) tau = __builtin_inff();  // NaN (a non-finite row or centroid norm) compares false: look everywhere
    if (!live) tau = -1.0f;

    // Rows arrive sorted by guess, so a 32-row tile holds a few runs of equal p: a group is needed by
    // the tile iff dmin[p][g] <= the largest tau of some run.  Lanes stand for groups here (64 per
    // pass, one coalesced read of the run's dmin row), not for rows.
    const long tile = wpos / 32;
    const bool second = wpos + 32 < n;
    int needed = 0;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        if (half == 1 && !second) break;
        const unsigned long long hm = half ? 0xffffffff00000000ull : 0x00000000ffffffffull;
        const bool mine = live && ((lane >> 5) == half);
        const bool all = (__builtin_amdgcn_ballot_w64(mine && !has) != 0);
        unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (all) {
#pragma unroll
            for (int it = 0; it < 8; it++) acc[it] = ~0ull;
        } else {
            unsigned long long todo = __builtin_amdgcn_ballot_w64(mine) & hm;
            while (todo != 0) {
                const int leader = __builtin_ctzll(todo);
                const uint32_t pl = (uint32_t)__builtin_amdgcn_readlane((int)p, leader);
                const bool in_run = mine && p == pl;
                todo &= ~__builtin_amdgcn_ballot_w64(in_run);
                float t = in_run ? tau : -1.0f;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) t = __builtin_fmaxf(t, __shfl_xor(t, off));
                const float* drow = dmin + (size_t)pl * ng;
#pragma unroll
                for (int it = 0; it < 8; it++) {
                    const int g = 64 * it + lane;
                    if (64 * it < ng) acc[it] |= __builtin_amdgcn_ballot_w64(g < ng && drow[g] <= t);
                }
            }
        }
#pragma unroll
        for (int it = 0; it < 8; it++) {
            if (64 * it >= ng) break;
            unsigned long long v = acc[it];
            if (ng - 64 * it < 64) v &= (1ull << (ng - 64 * it)) - 1ull;
            if (lane == 0) {
                mask[(size_t)(tile + half) * ngw + 2 * it] = (uint32_t)v;
                if (2 * it + 1 < ngw) mask[(size_t)(tile + half) * ngw + 2 * it + 1] = (uint32_t)(v >> 32);
            }
            needed += __builtin_popcountll(v);
        }
    }
    if (lane == 0) {  // statistics only (256 slots to keep the atomics off one address)
        unsigned long long* slot = stats + 2 * (blockIdx.x & 255);
        atomicAdd(&slot[0], (unsigned long long)needed);
        atomicAdd(&slot[1], (unsigned long long)ng * (second ? 2 : 1));
    }
}

// Coarse step of the unguided search: every row names one group (hint_sorted holds GROUP ids here);
// the tile needs exactly the groups its rows name, and nobody has a running best yet.
__global__ void __launch_bounds__(WG) group_only_mask_kernel(long n, const uint32_t* __restrict__ group_sorted,
                                                             int ng, const uint32_t* __restrict__ gnbr,
                                                             float* __restrict__ bd_out,
                                                             uint32_t* __restrict__ mask, int ngw) {
    const int lane = threadIdx.x & 63;
    const long wpos = ((long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6)) * 64;
    if (wpos >= n) return;
    const long pos = wpos + lane;
    const bool live = pos < n;
    const uint32_t g = live ? group_sorted[pos] : 0xffffffffu;
    if (live) bd_out[pos] = __builtin_inff();
    const long tile = wpos / 32;
    const bool second = wpos + 32 < n;
    for (int w = 0; w < ngw; w++) {
        // OR of (1 << bit) over the lanes of each half-wave whose group falls into word w
        // gnbr (optional, [ng][ngw]): the groups worth searching for a row that names group g
        uint32_t mine = 0u;
        if (live && g < (uint32_t)ng)
            mine = gnbr ? gnbr[(size_t)g * ngw + w] : ((int)(g >> 5) == w ? (1u << (g & 31)) : 0u);
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) mine |= (uint32_t)__shfl_xor((int)mine, off);
        if (lane == 0) mask[(size_t)tile * ngw + w] = mine;
        if (lane == 32 && second) mask[(size_t)(tile + 1) * ngw + w] = mine;
    }
}

// means[g] = mean of the group's member rows (coarse quantiser of the unguided search)
__global__ void __launch_bounds__(WG) group_means_kernel(const float* __restrict__ C, int d,
                                                         const int32_t* __restrict__ cperm,
                                                         float* __restrict__ means) {
    const int g = blockIdx.x;
    for (int f = threadIdx.x; f < d; f += WG) {
        float s = 0.0f;
        int cnt = 0;
        for (int m = 0; m < 32; m++) {
            const int row = cperm[g * 32 + m];
            if (row >= 0) { s += C[(size_t)row * d + f]; cnt++; }
        }
        means[(size_t)g * d + f] = cnt ? s / (float)cnt : 0.0f;
    }
}

// Neighbour table of the groups (heuristic input of the guess generators): one workgroup per group g
// scores every group mean against mean g (fp32 sum of squared differences), then takes the nnb nearest
// (g itself first; ties to the lower index) and sets their bits in gnbr[g][0..ngw).
__global__ __launch_bounds__(256) void group_neighbours_kernel(const float* __restrict__ means, int ng, int d, int nnb,
                                                               uint32_t* __restrict__ gnbr) {
    __shared__ float own[128];
    __shared__ unsigned long long wave_best[4];
    __shared__ uint32_t bits[16];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int ngw = (ng + 31) / 32;
    for (int f = tid; f < d; f += 256) own[f] = means[(size_t)g * d + f];
    if (tid < 16) bits[tid] = 0u;
    __syncthreads();
    // up to two candidates per thread (ng <= 512); key = distance bits (>= 0, so they order as integers) : index
    unsigned long long key[2];
    for (int s = 0; s < 2; s++) {
        const int j = tid + 256 * s;
        key[s] = ~0ull;
        if (j < ng && j != g) {
            float acc = 0.0f;
            for (int f = 0; f < d; f++) {
                const float t = means[(size_t)j * d + f] - own[f];
                acc = __builtin_fmaf(t, t, acc);
            }
            key[s] = ((unsigned long long)__float_as_uint(acc) << 32) | (unsigned)j;
        }
    }
    if (tid == 0) bits[g >> 5] |= 1u << (g & 31);
    for (int round = 1; round < nnb && round < ng; round++) {
        unsigned long long best = key[0] < key[1] ? key[0] : key[1];
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other < best ? other : best;
        }
        if ((tid & 63) == 0) wave_best[tid >> 6] = best;
        __syncthreads();
        best = wave_best[0];
        for (int w = 1; w < 4; w++) best = wave_best[w] < best ? wave_best[w] : best;
        __syncthreads();
        if (best == ~0ull) break;
        const unsigned j = (unsigned)best;
        if (tid == 0) bits[j >> 5] |= 1u << (j & 31);
        if (key[0] == best) key[0] = ~0ull;
        if (key[1] == best) key[1] = ~0ull;
    }
    __syncthreads();
    if (tid < ngw) gnbr[(size_t)g * ngw + tid] = bits[tid];
}

}  // namespace

// ---- entry points used by exact_search.cpp and the C ABI -------------------------------------------
int at_prune_prepass(at_ctx* ctx, const at_exact_call& call, int64_t n, const uint32_t* order, const uint32_t* hint_sorted,
                     int mode) {
    hipStream_t stream = call.stream;
    const long waves = (n + 63) / 64;
    const dim3 grid((unsigned)((waves + WG / 64 - 1) / (WG / 64)));
    ctx->prepass_n = n;
    ctx->prepass_ng = call.ng;
    if (mode == 1) {  // hint_sorted holds group ids: each tile needs just those groups (+ neighbours)
        AT_LAUNCH(group_only_mask_kernel, grid, dim3(WG), 0, stream, (long)n, hint_sorted, call.ng,
                  reinterpret_cast<const uint32_t*>(call.dmin), call.bd, call.mask, call.ngw);
        return AT_OK;
    }
    unsigned* cnmax = static_cast<unsigned*>(at_ws(ctx, WS_REDUCE, 1024 * sizeof(double), stream));
    if (!cnmax) return AT_E_NOMEM;
    AT_HIP(hipMemsetAsync(cnmax, 0, sizeof(unsigned), stream));
    AT_LAUNCH(max_sqnorm_kernel, dim3((call.k + WG - 1) / WG), dim3(WG), 0, stream, call.c, call.k, call.d, cnmax);
    const bool fresh = ctx->ws[WS_PRUNE_STATS] == nullptr;
    unsigned long long* stats = static_cast<unsigned long long*>(at_ws(ctx, WS_PRUNE_STATS, 4096, stream));
    if (!stats) return AT_E_NOMEM;
    if (fresh) AT_HIP(hipMemsetAsync(stats, 0, 4096, stream));
    if (call.d == 64)
        AT_LAUNCH(prune_mask_kernel<64>, grid, dim3(WG), 0, stream, call.x, (long)n, call.c, call.k, order, hint_sorted,
                  call.dmin, call.ng, cnmax, call.bd, call.mask, call.ngw, stats);
    else
        AT_LAUNCH(prune_mask_kernel<128>, grid, dim3(WG), 0, stream, call.x, (long)n, call.c, call.k, order, hint_sorted,
                  call.dmin, call.ng, cnmax, call.bd, call.mask, call.ngw, stats);
    return AT_OK;
}

// The block schedules of the order being made (at_internal.h: at_block_sched_state).  begin: the half of the workspace
// this call writes, claimed and entered on the stream of the visiting order; *weight = where key_to_hint_kernel puts the
// tile weights.  finish: the counting sort of the three tables, three small launches behind that kernel.
// The visiting order sits on the critical path of a Lloyd iteration (the next sweep waits for it), so what is queued
// behind the sort costs the step time: DESIGN.md section 5.0f lists the forms that were tried and cost more than this one
// (the sort on a stream of the context's own, one workgroup per table, class counts by atomics in key_to_hint_kernel).
// begin can stall that chain twice, both rarely: at_ws drains the device when the slot has to grow (until it has reached
// the largest n of the run), and a call whose n differs from the last one's enters both guards and drops both tags --
// a run that alternates Lloyd-sized and tokenise-sized orders lays the slot out anew at every switch (a wait only if a
// sweep on another stream still reads a half, which the Lloyd loop's joins exclude).
static int block_schedules_begin(at_ctx* ctx, int64_t n, const uint32_t* order_out, hipStream_t stream, unsigned char** weight) {
    at_block_sched_state& s = ctx->sched;
    const exact_plan::SchedLayout l = exact_plan::sched_layout(n);
    const int half = (int)(s.calls & 1u);
    if (s.layout_n != n) {   // the halves move: nobody may still be reading either, and neither holds a table any more
        for (int h = 0; h < 2; h++) {
            const int rc = at_guard_enter(&s.guard[h], stream);
            if (rc) return rc;
            s.tag[h].valid = 0;
        }
        s.layout_n = 0;
    }
    s.tag[half].valid = 0;
    if (s.tag[half ^ 1].order == order_out) s.tag[half ^ 1].valid = 0;   // (the buffer holds another order now)
    unsigned char* slot = static_cast<unsigned char*>(at_ws(ctx, WS_BLOCK_SCHED, 2 * l.bytes, stream));
    if (!slot) return AT_E_NOMEM;
    s.layout_n = n;
    const int rc = at_guard_enter(&s.guard[half], stream);   // a sweep on another stream may still read this half
    if (rc) return rc;
    *weight = slot + (size_t)half * l.bytes + l.weight_off;
    return AT_OK;
}

static int block_schedules_finish(at_ctx* ctx, int64_t n, const uint32_t* order_out, hipStream_t stream) {
    at_block_sched_state& s = ctx->sched;
    const exact_plan::SchedLayout l = exact_plan::sched_layout(n);
    const int half = (int)(s.calls & 1u);
    unsigned char* base = static_cast<unsigned char*>(ctx->ws[WS_BLOCK_SCHED]) + (size_t)half * l.bytes;
    const unsigned char* weight = base + l.weight_off;
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + l.hist_off);
    uint32_t* table[3];
    for (int t = 0; t < 3; t++) table[t] = reinterpret_cast<uint32_t*>(base + l.table_off[t]);
    const dim3 grid((unsigned)l.chunks, 3);
    AT_LAUNCH(sched_hist_kernel, grid, dim3(WG), 0, stream, weight, (long)l.tiles, (long)l.chunks, hist);
    AT_LAUNCH(sched_scan_kernel, dim3(3), dim3(WG), 0, stream, (long)l.tiles, (long)l.chunks, hist);
    AT_LAUNCH(sched_scatter_kernel, grid, dim3(WG), 0, stream, weight, (long)l.tiles, (long)l.chunks, hist, table[0], table[1],
              table[2]);
    const int rc = at_guard_leave(&s.guard[half], stream);
    if (rc) return rc;
    s.tag[half] = exact_plan::SchedTag{order_out, n, 1};
    s.calls++;
    return AT_OK;
}

extern "C" {

int at_group_min_dist_f32(at_ctx* ctx, const float* c, int k, int d, const int32_t* cperm, int ng,
                          float* dmin, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx && c && cperm && dmin && k > 0 && d > 0 && ng > 0, "at_group_min_dist_f32: bad arguments");
    AT_REQUIRE((d == 64 || d == 128) && at_aligned16(c), "at_group_min_dist_f32: d must be 64 or 128");
    AT_HIP(hipSetDevice(ctx->device));
    if (ctx->dbg.dmin_kernel != 0) return   // (switch: 0 = the fp32 vector-ALU kernel below)
        at_group_min_dist_f16(ctx, c, k, d, cperm, ng, dmin, stream);
    ctx->img16_c = nullptr;  // (no fp16 image is left behind by this form)
    const dim3 grid(ng, (k + WG - 1) / WG);
    if (d == 64)
        AT_LAUNCH(group_min_dist_kernel<64>, grid, dim3(WG), 0, stream, c, k, cperm, ng, dmin);
    else
        AT_LAUNCH(group_min_dist_kernel<128>, grid, dim3(WG), 0, stream, c, k, cperm, ng, dmin);
    return AT_OK;
}

int at_prune_stats(at_ctx* ctx, int64_t* needed, int64_t* total, int reset) {
    AT_REQUIRE(ctx && needed && total, "at_prune_stats: bad arguments");
    *needed = *total = 0;
    if (!ctx->ws[WS_PRUNE_STATS]) return AT_OK;
    AT_HIP(hipSetDevice(ctx->device));
    unsigned long long host[512];
    AT_HIP(hipDeviceSynchronize());
    AT_HIP(hipMemcpy(host, ctx->ws[WS_PRUNE_STATS], sizeof host, hipMemcpyDeviceToHost));
    for (int i = 0; i < 256; i++) {
        *needed += (int64_t)host[2 * i];
        *total += (int64_t)host[2 * i + 1];
    }
    if (reset) AT_HIP(hipMemset(ctx->ws[WS_PRUNE_STATS], 0, 4096));
    return AT_OK;
}

int at_group_means_f32(at_ctx* ctx, const float* c, int k, int d, const int32_t* cperm, int ng, float* means,
                       void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx && c && cperm && means && k > 0 && d > 0 && ng > 0, "at_group_means_f32: bad arguments");
    AT_HIP(hipSetDevice(ctx->device));
    AT_LAUNCH(group_means_kernel, dim3(ng), dim3(WG), 0, stream, c, d, cperm, means);
    return AT_OK;
}

int at_group_neighbours_f32(at_ctx* ctx, const float* means, int ng, int d, int nnb, uint32_t* gnbr, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx && means && gnbr, "at_group_neighbours_f32: null pointer");
    AT_REQUIRE(ng > 0 && ng <= 512 && d > 0 && d <= 128 && nnb > 0, "at_group_neighbours_f32: needs ng <= 512, d <= 128, nnb > 0");
    AT_HIP(hipSetDevice(ctx->device));
    AT_LAUNCH(group_neighbours_kernel, dim3(ng), dim3(256), 0, stream, means, ng, d, nnb, gnbr);
    return AT_OK;
}

int at_visit_order_f32(at_ctx* ctx, const int64_t* ids, const float* dis, int64_t n, int k,
                       uint32_t* order_out, uint32_t* hint_sorted_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx && ids && order_out && hint_sorted_out, "at_visit_order_f32: null pointer");
    AT_REQUIRE(n >= 0 && n < (int64_t)UINT32_MAX && k > 0 && k < (1 << 23), "at_visit_order_f32: bad sizes");
    if (n == 0) return AT_OK;
    AT_HIP(hipSetDevice(ctx->device));
    uint32_t* keys_a = static_cast<uint32_t*>(at_ws(ctx, WS_VISIT_KEYS_A, (size_t)n * 4, stream));
    uint32_t* keys_b = static_cast<uint32_t*>(at_ws(ctx, WS_VISIT_KEYS_B, (size_t)n * 4, stream));
    uint32_t* vals_a = static_cast<uint32_t*>(at_ws(ctx, WS_VISIT_VALS_A, (size_t)n * 4, stream));
    uint32_t* vals_b = static_cast<uint32_t*>(at_ws(ctx, WS_VISIT_VALS_B, (size_t)n * 4, stream));
    if (!keys_a || !keys_b || !vals_a || !vals_b) return AT_E_NOMEM;
    // key = cluster | distance in `dbits` bits (switch visit_bits, default 8: measured 2.07 / 1.86 / 1.52 / 1.46 ms per
    // Lloyd iteration at 0 / 2 / 5 / 8 bits on bench-like rows, no further gain at 10 or 12)
    unsigned cbits = 1;
    while ((1u << cbits) <= (unsigned)k) cbits++;
    int dbits = ctx->dbg.visit_bits;
    if (dbits < 0) dbits = 0;
    if (dbits > 12) dbits = 12;
    if ((int)cbits + dbits > 32) dbits = 32 - (int)cbits;
    AT_LAUNCH(visit_keys_kernel, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, stream,
                       reinterpret_cast<const long*>(ids), dis, (long)n, k, keys_a, vals_a, dbits);
    const unsigned bits = cbits + (unsigned)dbits;
    rocprim::double_buffer<uint32_t> kb(keys_a, keys_b);
    rocprim::double_buffer<uint32_t> vb(vals_a, vals_b);
    { const int rc = at_sort_pairs(ctx, WS_VISIT_TMP, kb, vb, (size_t)n, 0, bits, stream); if (rc != AT_OK) return rc; }
    // (switch block_sched: 0 = no tables are made, the sweeps start their blocks in visiting order)
    unsigned char* weight = nullptr;
    if (ctx->dbg.block_sched != 0) {
        const int rc = block_schedules_begin(ctx, n, order_out, stream, &weight);
        if (rc != AT_OK) return rc;
    }
    AT_LAUNCH(key_to_hint_kernel, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, stream, kb.current(),
                       vb.current(), (long)n, hint_sorted_out, order_out, dbits, k, weight);
    if (weight) return block_schedules_finish(ctx, n, order_out, stream);
    return AT_OK;
}

}  // extern "C"
