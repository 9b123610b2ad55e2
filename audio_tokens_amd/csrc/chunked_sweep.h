// chunked_sweep.h -- the chunked centroid image and the dense sweep over it, once.
//
// The image (built by at_prep_chunked_image, assign.hip): tiles of 32 * na centroid rows; the feature axis cut into
// chunks of DC = 64; a tile is its chunks one after the other ("pieces" of 32 * na rows x 64 floats), followed by the
// CN_PAD squared norms of its rows (+inf for rows >= k, so a pad row never wins an L2 search).  A row piece is 16 slots
// of 16 bytes; logical slot 2 q + h holds the features 8 q + {0, 2, 4, 6} + h of the chunk -- the A operands of four
// consecutive v_mfma_f32_32x32x2_f32 of half-wave h -- and sits at physical slot chunk_slot(row, q, h), XOR-swizzled by
// the row so that the 16-byte LDS reads of a wave are conflict free.  Producer and readers share that one function.
//
// The sweep (ip.hip and rq.hip through Sweep::run with a functor for the finished tile; knn.hip writes its own stage
// from begin_stage / mfma_piece, see there): a workgroup of 4 waves streams the pieces through double-buffered LDS by LDS-DMA
// while each wave keeps 32 x rows as the MFMA B operand (lane l: row l & 31, the features of parity l >> 5).  The na
// accumulators of a tile stay live across its chunks, so every inner product is ONE ascending fmaf chain.  A finished
// accumulator register e of accumulator a of tile t holds centroid acc_base(t * na + a, h) + reg_offset(e): ascending
// in the code for a fixed half-wave, which is what the strict `<` / `>` tie rules of the consumers rest on.
//
// The layout functions are __host__ __device__ and compile with a plain host compiler
// (tests/test_chunked_layout_host.py).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define CS_HD __host__ __device__ __forceinline__
#else
#define CS_HD inline
#endif

namespace cs {

constexpr int DC = 64;        // features per chunk
constexpr int CN_PAD = 256;   // floats reserved per tile for the squared norms (whole 1 KiB pieces)
constexpr unsigned NONE = 0xffffffffu;   // "no centroid yet": the highest code and the highest index

CS_HD constexpr int tile_rows(int na) { return 32 * na; }
CS_HD constexpr int nchunks_of(int d) { return (d + DC - 1) / DC; }
CS_HD constexpr int piece_floats(int na) { return tile_rows(na) * DC; }            // one (tile, chunk) piece
CS_HD constexpr int buf_floats(int na) { return piece_floats(na) + CN_PAD; }       // + the norms behind the last chunk
CS_HD constexpr size_t tile_floats(int na, int nchunks) { return (size_t)piece_floats(na) * nchunks + CN_PAD; }

// physical 16-byte slot, within the 64 floats of row r of a piece, of the features 8 q + {0, 2, 4, 6} + h
CS_HD constexpr int chunk_slot(int r, int q, int h) { return (2 * q + h) ^ (r & 15); }

// Register e of accumulator ai = tile * na + accumulator holds, in half-wave h, centroid
// acc_base(ai, h) + reg_offset(e);
// centroid_of: the same from the code ai * 16 + e that the running minima keep.  (Two functions, so that a sweep takes
// the lane's base once per accumulator and adds sixteen constants.)
CS_HD constexpr int acc_base(int ai, int h) { return ai * 32 + 4 * h; }
CS_HD constexpr int reg_offset(int e) { return (e & 3) + 8 * (e >> 2); }
CS_HD constexpr unsigned centroid_of(unsigned code, int h) {
    return (unsigned)(acc_base((int)(code >> 4), h) + reg_offset((int)(code & 15u)));
}

}  // namespace cs

// floats per tile of the image of d-feature centroids
static inline size_t at_chunked_image_tile_floats(int d, int na) { return cs::tile_floats(na, cs::nchunks_of(d)); }

#if defined(__HIPCC__)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace cs {

// 1 KiB of global memory -> LDS without passing through registers (global_load_lds_dwordx4):
// lane l's 16 bytes land at lds_wave_base + 16*l.
__device__ __forceinline__ void dma_1k(const float* gsrc_lane, float* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc_lane,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// the orc_assign clamp of knn / pq / rq: a NaN stays a NaN (assign.hip clamps with fmaxf, which makes it 0)
__device__ __forceinline__ float clamp0(float v) { return v < 0.0f ? 0.0f : v; }

// ---- the x side ----------------------------------------------------------------------------------------------------
// |x|^2 of a row of d features (d % 4 == 0): the ascending chain over 16-byte loads
__device__ __forceinline__ float sqnorm16(const float* xrow, int d) {
    float xn = 0.0f;
    for (int f = 0; f < d; f += 4) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(xrow + f);
        xn = __builtin_fmaf(u[0], u[0], xn);
        xn = __builtin_fmaf(u[1], u[1], xn);
        xn = __builtin_fmaf(u[2], u[2], xn);
        xn = __builtin_fmaf(u[3], u[3], xn);
    }
    return xn;
}

// chunk ch of a row of d features (d % 4 == 0, `pad` past d) as the B operand of half-wave h: xv[i] = feature 2 i + h.
// pad = +0 is enough wherever the sign of a zero product is never seen (the L2 routes: fma(-2, +-0, xn + cn) is the
// same number); ip.hip reports the product itself and pads with -0: against the image's +0 a pad step then adds -0,
// which leaves every accumulator as it is, a -0 included (+0 would turn it into +0).
__device__ __forceinline__ void load_x_chunk(const float* xrow, int ch, int d, int h, float (&xv)[DC / 2],
                                             float pad = 0.0f) {
#pragma unroll
    for (int q = 0; q < DC / 8; q++) {
        const int f = ch * DC + 8 * q;
        f32x4 u = {pad, pad, pad, pad}, v = {pad, pad, pad, pad};
        if (f < d) u = *reinterpret_cast<const f32x4*>(xrow + f);
        if (f + 4 < d) v = *reinterpret_cast<const f32x4*>(xrow + f + 4);
        xv[4 * q + 0] = h ? u[1] : u[0];
        xv[4 * q + 1] = h ? u[3] : u[2];
        xv[4 * q + 2] = h ? v[1] : v[0];
        xv[4 * q + 3] = h ? v[3] : v[2];
    }
}

// ---- the producer side ---------------------------------------------------------------------------------------------
// The 16 bytes of physical slot pc of image row r, from centroid crow (nullptr: a pad row) and the features from f0 on:
// the swizzle is an involution, so slot pc holds logical slot lc = chunk_slot(r, pc >> 1, pc & 1).
__device__ __forceinline__ f32x4 image_slot(const float* crow, int d, int f0, int r, int pc) {
    const int lc = chunk_slot(r, pc >> 1, pc & 1);
    const int q = lc >> 1, h = lc & 1;
    f32x4 v;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int f = f0 + 8 * q + 2 * u + h;
        v[u] = (crow && f < d) ? crow[f] : 0.0f;
    }
    return v;
}

// |c|^2 as the ascending fmaf chain; +inf for a pad row
__device__ __forceinline__ float image_norm(const float* crow, int d) {
    if (!crow) return __builtin_inff();
    float nrm = 0.0f;
    for (int f = 0; f < d; f++) nrm = __builtin_fmaf(crow[f], crow[f], nrm);
    return nrm;
}

// ---- the sweep -----------------------------------------------------------------------------------------------------
// NA accumulators per tile; NCH > 0: d = 64 * NCH and the x chunks stay in registers, NCH = 0: any d % 4 == 0 and the x
// chunk is re-read per piece; NORMS: the last chunk of a tile drags the tile's norms along into LDS.
// The stream is the tiles [0, ntiles) of the image, piece s = tile * nch + chunk in LDS buffer s & 1.  prime() issues
// piece 0; run(t0, t1, ...) consumes the tiles [t0, t1) and issues the piece behind each one it consumes, so
// consecutive run() calls continue one stream without re-priming and the next piece is in flight between them.
template <int NA, int NCH, bool NORMS>
struct Sweep {
    static_assert(NCH >= 0 && NCH <= 2, "x chunks held in registers: d = 64 or 128");
    static constexpr int PIECE_F = piece_floats(NA);
    static constexpr int STRIDE_F = NORMS ? buf_floats(NA) : PIECE_F;   // floats per LDS buffer (two of them)

    const float* img;
    float* smem;
    int nch, nstages;
    int lane, wave, j, h;
    size_t tile_f;

    __device__ __forceinline__ Sweep(const float* img_, float* smem_, int nchunks, int ntiles)
        : img(img_), smem(smem_) {
        lane = threadIdx.x & 63;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        j = lane & 31;   // x row within the wave's 32 rows == accumulator column
        h = lane >> 5;   // which k of each MFMA k-pair this lane feeds
        nch = NCH > 0 ? NCH : nchunks;
        nstages = ntiles * nch;
        tile_f = tile_floats(NA, nch);
    }

    __device__ __forceinline__ void issue(int ct, int ch, float* dst) const {
        const float* src = img + (size_t)ct * tile_f + (size_t)ch * PIECE_F;
        const int pieces = (NORMS && ch == nch - 1 ? buf_floats(NA) : PIECE_F) / 256;
        for (int p = wave; p < pieces; p += 4) dma_1k(src + p * 256 + lane * 4, dst + p * 256);
    }

    __device__ __forceinline__ void prime() const {
        issue(0, 0, smem);
        __syncthreads();
    }

    // acc (+)= piece x chunk (first: the tile's first chunk, acc starts from +0): per accumulator 32 MFMAs whose k
    // order is the ascending feature order.  The accumulators are the caller's, a local array.
    __device__ __forceinline__ void mfma_piece(f32x16 (&acc)[NA], const float* cur, const float (&xv)[DC / 2],
                                               bool first) const {
#pragma unroll
        for (int a = 0; a < NA; a++) {
            const float* arow = cur + (a * 32 + j) * DC;
            f32x16 cacc = acc[a];
            if (first) cacc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < DC / 8; q++) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(arow + chunk_slot(j, q, h) * 4);
                cacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], xv[4 * q + 0], cacc, 0, 0, 0);
                cacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], xv[4 * q + 1], cacc, 0, 0, 0);
                cacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], xv[4 * q + 2], cacc, 0, 0, 0);
                cacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], xv[4 * q + 3], cacc, 0, 0, 0);
            }
            acc[a] = cacc;
        }
    }

    // piece s = (tile ct, chunk ch): issues the piece behind it and returns the LDS buffer of this one; the caller ends
    // the stage with __syncthreads().  lds: the two buffers (smem; a kernel that writes its own stage passes its LDS
    // array itself, which saves the keys kernel of knn.hip two registers over the copy held here).
    __device__ __forceinline__ const float* begin_stage(float* lds, int s, int ct, int ch) const {
        const float* cur = lds + (s & 1) * STRIDE_F;
        if (s + 1 < nstages) {
            const bool wrap = ch + 1 == nch;
            issue(wrap ? ct + 1 : ct, wrap ? 0 : ch + 1, lds + ((s + 1) & 1) * STRIDE_F);
        }
        return cur;
    }

    // one stage; done(ct, the tile's norms in LDS, acc) behind the tile's last chunk
    template <typename F>
    __device__ __forceinline__ void stage(int s, int ct, int ch, f32x16 (&acc)[NA], const float (&xv)[DC / 2],
                                          F& done) const {
        const float* cur = begin_stage(smem, s, ct, ch);
        mfma_piece(acc, cur, xv, ch == 0);
        if (ch == nch - 1) done(ct, cur + PIECE_F, acc);
        __syncthreads();
    }

    // NCH > 0: xr holds the row's chunks; NCH = 0: xr[0] is reloaded from xrow (d features, xpad behind them) for
    // every piece
    template <typename F>
    __device__ __forceinline__ void run(int t0, int t1, f32x16 (&acc)[NA], float (&xr)[NCH > 0 ? NCH : 1][DC / 2],
                                        const float* xrow, int d, F&& done, float xpad = 0.0f) const {
        if constexpr (NCH > 0) {
            for (int ct = t0; ct < t1; ct++) {   // (written out: a chunk index must be a constant here)
                stage(ct * NCH, ct, 0, acc, xr[0], done);
                if constexpr (NCH == 2) stage(ct * NCH + 1, ct, 1, acc, xr[NCH - 1], done);
            }
        } else {
            int ct = t0, ch = 0;
            for (int s = t0 * nch; s < t1 * nch; s++) {
                load_x_chunk(xrow, ch, d, h, xr[0], xpad);
                stage(s, ct, ch, acc, xr[0], done);
                if (++ch == nch) { ch = 0; ct++; }
            }
        }
    }
};

// ---- one centroid per row out of the two half-waves (same rows, disjoint centroids) --------------------------------
// code -> index; NONE stays NONE (the highest index)
__device__ __forceinline__ unsigned index_of(unsigned code, int h) {
    return code != NONE ? centroid_of(code, h) : NONE;
}

// the smaller value, the lower index on equal values
__device__ __forceinline__ void merge_halves_min(float& v, unsigned& idx) {
    const float ov = __shfl_xor(v, 32);
    const unsigned oi = (unsigned)__shfl_xor((int)idx, 32);
    if (ov < v || (ov == v && oi < idx)) {
        v = ov;
        idx = oi;
    }
}

// the larger value, the lower index on equal values
__device__ __forceinline__ void merge_halves_max(float& v, unsigned& idx) {
    const float ov = __shfl_xor(v, 32);
    const unsigned oi = (unsigned)__shfl_xor((int)idx, 32);
    if (ov > v || (ov == v && oi < idx)) {
        v = ov;
        idx = oi;
    }
}

// ---- code selection of the quantisers (pq.hip, rq.hip) -------------------------------------------------------------
// Running strict `<` minimum over the 16 registers of a finished accumulator, met in ascending index:
// dis = clamp0(fma(-2, acc, xn + cn)); cnh: the norms of the accumulator's 32 centroids from this half-wave's first
// one on (+ 4 h: taken once per tile by the caller, as a pointer), code = codebase + register.
__device__ __forceinline__ void min16(const f32x16& acc, const float* cnh, float xn, unsigned codebase, float& best,
                                      unsigned& bcode) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(cnh + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float v = clamp0(__builtin_fmaf(-2.0f, acc[4 * g + e], xn + c[e]));
            const bool lt = v < best;   // false for a NaN and for +inf
            best = lt ? v : best;
            bcode = lt ? codebase + (unsigned)(4 * g + e) : bcode;
        }
    }
}

// Merges the half-waves' (best, bcode): best becomes the row's distance; returns its centroid, NONE if nothing was
// listed (best is still +inf).
__device__ __forceinline__ unsigned merged_index(float& best, unsigned bcode, int h) {
    unsigned idx = index_of(bcode, h);
    merge_halves_min(best, idx);
    return idx;
}

// Where the codes of a call go.  put(): lanes with `store` write element o = row * M + m -- the distance, and the code
// as a byte or (pack4) as one 32-bit store per four codes, collected in `pack`; nothing listed (idx == NONE): code 0
// and *bad raised.  Returns the code.
struct CodeSink {
    uint8_t* codes;
    float* dist;
    int* bad;
    int pack4;

    __device__ __forceinline__ unsigned put(unsigned idx, float best, bool store, long o, int m, unsigned& pack) const {
        const bool none = idx == NONE;
        if (none) idx = 0u;
        if (store) {
            if (dist) dist[o] = best;
            if (none && bad) *bad = 1;
            if (pack4) {
                pack |= idx << (8 * (m & 3));
                if ((m & 3) == 3) {
                    *reinterpret_cast<unsigned*>(codes + o - 3) = pack;
                    pack = 0;
                }
            } else {
                codes[o] = (uint8_t)idx;
            }
        }
        return idx;
    }
};

}  // namespace cs

#endif  // __HIPCC__
