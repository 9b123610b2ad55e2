// logmel.hip -- fused waveform -> STFT -> |.|^2 -> mel -> dB on gfx950 (at_logmel_f32).
//
// Replaces SpectrogramGenerator.generate_mel_spectrogram (processors/spectrogram_generator.py:
// 123-126 of danavery/audio-tokens): torchaudio MelSpectrogram(sample_rate, n_mels, n_fft=512,
// hop_length) with its defaults (center=True, reflect padding, periodic Hann, power=2, htk mel
// scale, norm=None, f_min=0, f_max=sr//2) followed by AmplitudeToDB() (10*log10(max(x, 1e-10))).
// Optionally emits frame-major rows and the row L2 normalisation the two consumers apply next
// (cluster_creator.py:52,64-66; spec_tokenizer.py:76,106-109), which removes the reference's
// transpose + normalise round trip through memory.
//
// One workgroup = FPB consecutive frames of one clip.  Their samples are read from HBM once,
// coalesced, into LDS with the reflect padding applied on the way (every sample is shared by
// n_fft/hop = 4 frames).  A frame is owned by 16 lanes (4 frames per wavefront): 16-point FFTs
// in registers down the columns, one transpose through a conflict-free LDS tile, 16-point FFTs
// along the rows, even/odd untangling to the 257 power bins (logmel_core.h), then the mel
// filterbank as a banded dot product per filter (only the non-zero taps), 10*log10, and a staged
// coalesced store.  Algorithmic HBM traffic: hop*4 bytes in + n_mels*4 bytes out per frame.
//
// Whose clip a block is, and where that clip lies, is the clip map's business (logmel_clips.h): the uniform batch of
// at_logmel_f32 and the plan of at_logmel_ragged_f32 are two instantiations of the same kernel, of the same min-max
// passes and of the same host driver (logmel_drive), which also sends every other n_fft to logmel_any.hip.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "at_internal.h"
#include "l2norm_core.h"
#include "logmel_clips.h"
#include "logmel_core.h"
#include "logmel_tables.h"

namespace {

using namespace logmel;

constexpr int WG = 256;
constexpr int PREFETCH_REGS = 5;   // x 16 bytes x 256 lanes = 5120 samples per block: 32 frames at hop <= 148, 16 at hop <= 307
constexpr int TAB_WIN = 0, TAB_TW256 = 512, TAB_TW512 = 1024, TAB_FLOATS = 1536;
// A frame's LDS tile (FRAME_LDS_FLOATS = 2304 B) is a multiple of the 256-byte bank row, so the two frames of a half-wave
// hit the same banks with every 64-bit tile access; 128 bytes of slack between tiles put neighbouring frames on
// opposite halves of the banks.
constexpr int FRAME_STRIDE = FRAME_LDS_FLOATS + 32;

// What the kernel needs beside the clips: the tables, the block geometry and where the output goes.
struct LogmelCommon {
    int hop, n_mels, fpb;
    long n_blocks;          // (clip, block of fpb frames) pairs, walked by persistent workgroups
    const float* tabs;      // TAB_FLOATS floats: window, W256 twiddles, W512 twiddles
    const int* fb_start;    // [n_mels]
    const int* fb_len;      // [n_mels]
    const int* fb_off;      // [n_mels] offset into fb_wts
    const float* fb_wts;    // concatenated non-zero bands
    int fb_nw;              // number of weights; tables are copied to LDS when fb_lds != 0
    int fb_lds;
    int fb_quads;           // bands padded to 4-aligned quads of bins (16-byte reads) or stored as they are
    float* out;
    int frame_major, fuse_l2norm;
    int* bad;               // set to 1 when a frame's squared norm is not finite (fused unit rows only)
    unsigned* minmax;       // optional [n_clips][4]: ordered keys of the clip's smallest / largest dB value, a NaN flag
                            // (the min-max entries: SpectrogramGenerator's normalize option without a reduction pass)
};
// Clips: the map from a block to its clip (logmel_clips.h)
template <typename Clips>
struct LogmelParams : LogmelCommon {
    Clips clips;
};

__device__ __forceinline__ int not_finite(float v) { return !(__builtin_fabsf(v) < __builtin_inff()); }

// floats as unsigned keys that order the same way (atomicMin / atomicMax on them)
__device__ __forceinline__ unsigned ordered_key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_to_float(unsigned kx) {
    return __uint_as_float((kx & 0x80000000u) ? (kx & 0x7fffffffu) : ~kx);
}

__global__ void __launch_bounds__(256) minmax_init_kernel(unsigned* __restrict__ mm, long n_clips) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c < n_clips) {
        mm[4 * c] = 0xffffffffu;   // smallest key seen
        mm[4 * c + 1] = 0u;        // largest
        mm[4 * c + 2] = 0u;        // a NaN was seen
        mm[4 * c + 3] = 0u;
    }
}

// A wavefront's (lo, hi, nan) of values of one clip, folded into the clip's record `rec` (minmax_init_kernel's): one
// pair of atomics per call.  Lanes that saw nothing bring +inf / -inf / 0.
__device__ __forceinline__ void commit_extremes(unsigned* rec, float lo, float hi, int nan, int lane) {
    for (int off = 32; off > 0; off >>= 1) {
        lo = __builtin_fminf(lo, __shfl_xor(lo, off));
        hi = __builtin_fmaxf(hi, __shfl_xor(hi, off));
        nan |= __shfl_xor(nan, off);
    }
    if (lane == 0) {
        if (lo <= hi) {
            atomicMin(&rec[0], ordered_key(lo));
            atomicMax(&rec[1], ordered_key(hi));
        }
        if (nan) atomicOr(&rec[2], 1u);
    }
}

// ---- the passes over a finished output (the min-max entries) -----------------------------------------------------------
// The output of either clip map is one flat run of floats in either layout: a clip owns [base, base + T) x n_mels of
// it.  A wavefront takes MM_CHUNK consecutive floats at a time and walks the pieces of clips inside them: a piece
// belongs to the clip that owns its first frame and ends where that clip or the chunk does (lmc::clip_end).
// Everything that decides the walk is the same in all 64 lanes.
constexpr int MM_CHUNK = 4096;
template <typename Clips>
struct MinmaxParams {
    float* x;                       // [n_frames][n_mels] floats, clip after clip
    long total;                     // n_frames * n_mels
    int n_mels, vec;                // vec: n_mels % 4 == 0 and x 16-byte aligned, so every piece is whole aligned quads
    Clips clips;
    unsigned* mm;                   // [n_clips][4] records, as minmax_init_kernel leaves them
};
template <typename Clips, typename Body>
__device__ __forceinline__ void clip_pieces(const MinmaxParams<Clips>& p, Body body) {
    const int lane = threadIdx.x & 63;
    const long wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const long n_waves = (long)gridDim.x * (blockDim.x >> 6);
    for (long a = wave * MM_CHUNK; a < p.total; a += n_waves * MM_CHUNK) {
        const long b = min(p.total, a + MM_CHUNK);
        for (long s = a; s < b;) {
            long clip;
            const long end = min(b, lmc::clip_end(p.clips, s / p.n_mels, &clip) * p.n_mels);
            if (end <= s) return;   // (a plan that does not cover the output: never loop on it)
            body(clip, s, end, lane);
            s = end;
        }
    }
}

// The reduction pass behind the transforms that do not collect the extremes themselves (every n_fft but 512): the same
// records, ordered keys and NaN flag as the tuned kernel leaves, one pair of atomics per piece.  4 B read per value.
template <typename Clips>
__global__ void __launch_bounds__(256) minmax_extremes_kernel(MinmaxParams<Clips> p) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    clip_pieces(p, [&](long clip, long s, long end, int lane) {
        float lo = __builtin_inff(), hi = -__builtin_inff();
        int nan = 0;
        if (p.vec) {
            const f4* x4 = reinterpret_cast<const f4*>(p.x);
            for (long q = (s >> 2) + lane; q < (end >> 2); q += 64) {
                const f4 v = x4[q];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    nan |= v[e] != v[e];
                    lo = __builtin_fminf(lo, v[e]);
                    hi = __builtin_fmaxf(hi, v[e]);
                }
            }
        } else {
            for (long e = s + lane; e < end; e += 64) {
                const float v = p.x[e];
                nan |= v != v;
                lo = __builtin_fminf(lo, v);
                hi = __builtin_fmaxf(hi, v);
            }
        }
        commit_extremes(p.mm + 4 * clip, lo, hi, nan, lane);
    });
}

// (spec - min) / (max - min) per clip with the extremes collected before, either layout: two subtractions and one
// IEEE division per value, torch's bits (processors/spectrogram_generator.py:129-131); a NaN anywhere in the clip
// makes the whole clip NaN, as torch.min / max propagate it.  A map with flags has a clip flagged where a value stored
// for it is not finite -- the reference checks for NaN / Inf after normalising
// (processors/spectrogram_generator.py:107-110), so a constant clip (0 / 0) is skipped like one with a NaN sample.
// 8 B per value.
template <typename Clips>
__global__ void __launch_bounds__(256) minmax_scale_pieces_kernel(MinmaxParams<Clips> p) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    clip_pieces(p, [&](long clip, long s, long end, int lane) {
        float lo = key_to_float(p.mm[4 * clip]), hi = key_to_float(p.mm[4 * clip + 1]);
        if (p.mm[4 * clip + 2]) lo = hi = __builtin_nanf("");
        const float range = hi - lo;
        int flagged = 0;
        if (p.vec) {
            f4* x4 = reinterpret_cast<f4*>(p.x);
            for (long q = (s >> 2) + lane; q < (end >> 2); q += 64) {
                f4 v = x4[q];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    v[e] = __fdiv_rn(v[e] - lo, range);
                    flagged |= not_finite(v[e]);
                }
                x4[q] = v;
            }
        } else {
            for (long e = s + lane; e < end; e += 64) {
                const float v = __fdiv_rn(p.x[e] - lo, range);
                flagged |= not_finite(v);
                p.x[e] = v;
            }
        }
        if constexpr (Clips::has_flags)
            if (flagged) p.clips.flags[clip] = 1;   // (every writer stores the same value)
    });
}

// PF: the next block's samples are prefetched through registers (needs a block of at most PREFETCH_REGS x WG x 4
// samples); otherwise they are staged at the top of the block.
// Clips: which clip a block belongs to (logmel_clips.h).
template <bool PF, typename Clips>
__global__ void __launch_bounds__(WG, 2) logmel_kernel(LogmelParams<Clips> p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, grp = lane >> 4;
    const int nsamp = (p.fpb - 1) * p.hop + NFFT;
    const int opitch = p.n_mels + 1;

    float* win = sm;                               // NFFT window values
    float* tw512 = win + NFFT;                     // 256 x (cos, -sin)
    float* samp = tw512 + NFFT;                    // nsamp (rounded up to 4)
    float* work = samp + ((nsamp + 3) & ~3);       // 16 frames x FRAME_LDS_FLOATS
    float* ostage = work + 16 * FRAME_STRIDE;      // fpb x opitch  (+ fpb denominators)
    // filterbank tables behind the staging area, 16-byte aligned: start4 | quads | off | padded weights
    int* fbi = reinterpret_cast<int*>(sm + ((2 * NFFT + ((nsamp + 3) & ~3) + 16 * FRAME_STRIDE + p.fpb * opitch + p.fpb + 3) & ~3));
    const int* fb_start = p.fb_start;
    const int* fb_len = p.fb_len;
    const int* fb_off = p.fb_off;
    const float* fb_wts = p.fb_wts;
    if (p.fb_lds) {
        const int nint = (3 * p.n_mels + 3) & ~3;
        for (int i = tid; i < nint + p.fb_nw; i += WG) fbi[i] = p.fb_start[i];  // one contiguous blob
        fb_start = fbi;
        fb_len = fbi + p.n_mels;
        fb_off = fbi + 2 * p.n_mels;
        fb_wts = reinterpret_cast<const float*>(fbi + nint);
    }
    // A lane's twiddles do not depend on the frame: they live in registers for the whole (persistent)
    // workgroup instead of being read from LDS once per frame (the window stays in LDS: the register file
    // does not hold more beside two 16-point FFTs; window and W512 stay in LDS).
    cpx twr[16];
#pragma unroll
    for (int k1 = 0; k1 < 16; k1++)
        twr[k1] = {p.tabs[TAB_TW256 + 2 * (k1 * 16 + l16)], p.tabs[TAB_TW256 + 2 * (k1 * 16 + l16) + 1]};
    for (int i = tid; i < NFFT; i += WG) {
        win[i] = p.tabs[TAB_WIN + i];
        tw512[i] = p.tabs[TAB_TW512 + i];
    }

    float* mybuf = work + (wave * 4 + grp) * FRAME_STRIDE;
    const int n_mel_iter = (p.n_mels + 15) >> 4;

    // The samples of a block travel global -> registers -> LDS: the loads of the NEXT block are issued
    // before this block's frames are computed and land in LDS after them, so their latency is not waited
    // for.  Blocks in the interior of a clip (no reflection, 16-byte aligned) move 16 bytes per lane.
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int nsamp4 = (nsamp + 3) >> 2;
    f4 pre[PREFETCH_REGS];
    auto prefetch = [&](long blk) {
        const lmc::ClipAt at = p.clips.by_block(blk, p.fpb);
        const float* w = at.w;
        const long s0 = (long)at.t * p.hop - NFFT / 2;
        const bool fast = s0 >= 0 && s0 + 4L * nsamp4 <= at.L && ((reinterpret_cast<uintptr_t>(w + s0) & 15) == 0);
        if (fast) {
            const f4* src = reinterpret_cast<const f4*>(w + s0);
#pragma unroll
            for (int j = 0; j < PREFETCH_REGS; j++) {
                const int i4 = tid + WG * j;
                if (i4 < nsamp4) pre[j] = src[i4];
            }
        } else {
#pragma unroll
            for (int j = 0; j < PREFETCH_REGS; j++) {
                const int i4 = tid + WG * j;
                if (i4 < nsamp4) {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        pre[j][e] = w[reflect_index(s0 + 4 * i4 + e, at.L)];
                    }
                }
            }
        }
    };
    if constexpr (PF)
        if ((long)blockIdx.x < p.n_blocks) prefetch(blockIdx.x);
    for (long blk = blockIdx.x; blk < p.n_blocks; blk += gridDim.x) {
        const lmc::ClipAt at = p.clips.by_block(blk, p.fpb);
        const long clip = at.clip;
        const int t0 = at.t;
        if constexpr (PF) {
#pragma unroll
            for (int j = 0; j < PREFETCH_REGS; j++) {
                const int i4 = tid + WG * j;
                if (i4 < nsamp4) *reinterpret_cast<f4*>(samp + 4 * i4) = pre[j];
            }
        } else {
            const float* w = at.w;
            const long s0 = (long)t0 * p.hop - NFFT / 2;
            for (int i = tid; i < nsamp; i += WG) samp[i] = w[reflect_index(s0 + i, at.L)];
        }
        __syncthreads();  // samples in place; the previous block's staged output has been stored by everybody
        if constexpr (PF)
            if (blk + gridDim.x < p.n_blocks) prefetch(blk + gridDim.x);

        for (int pass = 0; pass * 16 < p.fpb; pass++) {
            const int f = pass * 16 + wave * 4 + grp;   // frame within the workgroup
            // every DS access below stays inside this frame's 16 lanes' private tile; a wavefront's
            // LDS instructions execute in order, so no barrier is needed between the phases
            phase1_w(l16, samp + f * p.hop, win, twr, mybuf);
            cpx z[16];
            phase2(l16, mybuf, z);
            phase3_publish(l16, z, mybuf);
            float pw[16], p256 = 0.0f;
            phase3_power(l16, z, mybuf, tw512, pw, p256);
#pragma unroll
            for (int e = 0; e < 16; e++) mybuf[l16 + 16 * e] = pw[e];
            if (l16 < 4) mybuf[256 + l16] = l16 == 0 ? p256 : 0.0f;  // bins 257..259 pad the last quad
            for (int i = 0; i < n_mel_iter; i++) {
                const int m = l16 + 16 * i;
                if (m < p.n_mels) {
                    const float s = p.fb_quads ? mel_band(mybuf, fb_start[m], fb_len[m], fb_wts + fb_off[m])
                                               : mel_band_plain(mybuf, fb_start[m], fb_len[m], fb_wts + fb_off[m]);
                    // clamp(x, 1e-10) then 10*log10: a clamped bin is exactly -100 dB (what a correctly
                    // rounded log10 of 1e-10f gives; the device log10f is 1 ulp off there)
                    // (v_log_f32 is within an ulp of log2 on normal inputs -- s > 1e-10 here --: 1.2e-5 dB at most, a
                    // quarter of what the stated tolerance leaves; the library log10f costs twenty instructions)
                    ostage[f * opitch + m] = !(s <= 1e-10f) ? 3.0102999566398120f * __builtin_amdgcn_logf(s) : -100.0f;   // (a NaN power stays NaN, as torch.clamp leaves it)
                }
            }
        }
        __syncthreads();

        const int nf = min(p.fpb, at.T - t0);  // frames of this block that exist
        int flagged = 0;                      // (a map with flags) a value stored by this lane is not finite
        if (p.minmax) {   // the clip's extremes, from the staged block: one pair of atomics per workgroup and block
            float lo = __builtin_inff(), hi = -__builtin_inff();
            int nan = 0;
            for (int e = tid; e < nf * p.n_mels; e += WG) {
                const int f = e / p.n_mels, m = e - f * p.n_mels;
                const float v = ostage[f * opitch + m];
                nan |= v != v;
                lo = __builtin_fminf(lo, v);
                hi = __builtin_fmaxf(hi, v);
            }
            commit_extremes(p.minmax + 4 * clip, lo, hi, nan, lane);
        }
        if (p.frame_major) {
            float* den = ostage + p.fpb * opitch;
            if (p.fuse_l2norm) {
                // eight lanes per frame (fpb <= 32 frames: all of them at once); the host fuses only 8 <= n_mels <= 128
                const int f = tid >> 3;
                if (f < nf) {
                    const float ss = l2n::pairwise_sumsq_8lanes(ostage + f * opitch, p.n_mels, tid & 7);
                    if ((tid & 7) == 0) {
                        den[f] = __builtin_sqrtf(ss) + 1e-10f;
                        if (!(ss < __builtin_inff())) atomicOr(p.bad, 1);   // a NaN / Inf in the frame (faiss' input check, for free)
                    }
                }
                __syncthreads();
            }
            float* dst = p.out + (at.base + t0) * p.n_mels;
            if ((p.n_mels & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {   // 16 bytes per lane
                const int mq = p.n_mels >> 2, total4 = nf * mq;
                for (int e4 = tid; e4 < total4; e4 += WG) {
                    const int f = e4 / mq, m = (e4 - f * mq) * 4;
                    const float* src = ostage + f * opitch + m;
                    f4 v = {src[0], src[1], src[2], src[3]};
                    if (p.fuse_l2norm) {
                        const float dn = den[f];
#pragma unroll
                        for (int e = 0; e < 4; e++) v[e] = l2n::divide(v[e], dn);
                    }
                    if constexpr (Clips::has_flags) flagged |= not_finite(v[0]) | not_finite(v[1]) | not_finite(v[2]) | not_finite(v[3]);
                    reinterpret_cast<f4*>(dst)[e4] = v;
                }
            } else {
                const int total = nf * p.n_mels;
                for (int e = tid; e < total; e += WG) {
                    const int f = e / p.n_mels, m = e - f * p.n_mels;
                    float v = ostage[f * opitch + m];
                    if (p.fuse_l2norm) v = l2n::divide(v, den[f]);
                    if constexpr (Clips::has_flags) flagged |= not_finite(v);
                    dst[e] = v;
                }
            }
        } else {
            float* dst = p.out + at.base * p.n_mels + t0;
            const int total = p.n_mels * p.fpb;
            for (int e = tid; e < total; e += WG) {
                const int m = e / p.fpb, f = e - m * p.fpb;
                if (f < nf) {
                    const float v = ostage[f * opitch + m];
                    if constexpr (Clips::has_flags) flagged |= not_finite(v);
                    dst[(long)m * at.T + f] = v;
                }
            }
        }
        if constexpr (Clips::has_flags)
            if (flagged) p.clips.flags[clip] = 1;   // (every writer stores the same value)
        // (no barrier here: the next block's samples go to `samp`, which nobody reads any more, and its
        // barrier above comes before anybody writes the staged output again)
    }
}

// LDS bytes of one workgroup of `fpb` frames (kernel layout), with `fb_ints` words of filterbank tables
size_t lds_bytes(int fpb, int hop, int n_mels, size_t fb_ints) {
    const int nsamp = (fpb - 1) * hop + NFFT;
    return sizeof(float) * ((size_t)2 * NFFT + ((nsamp + 3) & ~3) + 16 * FRAME_STRIDE + (size_t)fpb * (n_mels + 1) + fpb) +
           fb_ints * 4 + 16;
}
constexpr size_t LDS_TWO_PER_CU = 80 * 1024;  // two workgroups of this size share a CU

// The blob of WS_LOGMEL_FB (an at_logmel_builder; `t` holds the key, and receives nw and quads): window | W256
// twiddles | W512 twiddles, then the banded filterbank (logmel_tables.h).  Bands padded with zero weights to whole
// 4-aligned quads of bins (16-byte LDS reads, see logmel_core.h mel_band) -- unless the padding is what pushes a
// 32-frame workgroup past half a CU's LDS, in which case the bands are stored as they are.  (A dense user filterbank,
// too big for LDS either way, stays in global memory: quads.)
void build_tables_512(const float* fb, std::vector<float>& blob, at_logmel_tables* t) {
    blob.assign(TAB_FLOATS, 0.0f);
    lmt::hann_periodic(NFFT, &blob[TAB_WIN]);
    for (int j = 0; j < 256; j++) {
        const int e = (j / 16) * (j % 16);  // layout [k1][m2] -> W256^(m2*k1) (logmel_core.h phase1)
        blob[TAB_TW256 + 2 * j] = (float)std::cos(2.0 * M_PI * e / 256.0);
        blob[TAB_TW256 + 2 * j + 1] = (float)-std::sin(2.0 * M_PI * e / 256.0);
        blob[TAB_TW512 + 2 * j] = (float)std::cos(2.0 * M_PI * j / 512.0);
        blob[TAB_TW512 + 2 * j + 1] = (float)-std::sin(2.0 * M_PI * j / 512.0);
    }
    for (int gran = 4;; gran = 1) {
        t->nw = (int)lmt::pack_bands(blob, TAB_FLOATS, fb, NBIN, t->nmels, gran);
        t->quads = gran == 4;
        const size_t words = lmt::table_ints(t->nmels) + t->nw;
        if (gran == 1 || lds_bytes(32, t->hop, t->nmels, words) <= LDS_TWO_PER_CU || words * 4 > 14 * 1024) break;
    }
}

}  // namespace

int at_logmel_resident(at_ctx* ctx, int slot, at_logmel_tables* rec, const at_logmel_tables& key, size_t cap_bytes,
                       const float* fb_user_dev, hipStream_t stream, const at_logmel_builder& build, const float** tabs) {
    const size_t fb_floats = (size_t)(key.nfft / 2 + 1) * key.nmels, fb_bytes = fb_floats * sizeof(float);
    std::vector<float> fb;
    if (fb_user_dev) {
        // A caller's filterbank is never trusted by address (allocators hand the same address to the next tensor of
        // the same shape, and a tensor can be rewritten in place): its VALUES are read back and compared with the copy
        // the resident tables were built from.  66 KB at 512 x 64 and one stream synchronisation per call -- the price
        // of the option; the library's own filterbank (fb_or_null == NULL) pays nothing.
        fb.resize(fb_floats);
        AT_HIP(hipStreamSynchronize(stream));
        AT_HIP(hipMemcpy(fb.data(), fb_user_dev, fb_bytes, hipMemcpyDeviceToHost));
    }
    // (a slot that at_ws regrew, or that a failed call left in flux, has an all-zero record: nmels = 0 matches no call)
    const bool hit = ctx->ws[slot] && rec->sr == key.sr && rec->nfft == key.nfft && rec->nmels == key.nmels &&
                     rec->hop == key.hop && rec->form == key.form && (rec->user_copy != nullptr) == (fb_user_dev != nullptr) &&
                     (!fb_user_dev || std::memcmp(rec->user_copy, fb.data(), fb_bytes) == 0);
    if (hit) {
        *tabs = static_cast<const float*>(ctx->ws[slot]);
        return AT_OK;
    }
    if (!fb_user_dev) {
        fb.resize(fb_floats);
        int rc = at_mel_filterbank_host(key.sr, key.nfft, key.nmels, fb.data());
        if (rc) return rc;
    }
    // Everything that can fail for want of memory comes first, while the slot and its record are still whole ...
    std::vector<float> blob;
    at_logmel_tables filled = key;
    build(fb.data(), blob, &filled);
    std::unique_ptr<float, decltype(&std::free)> copy(nullptr, &std::free);
    if (fb_user_dev) {
        copy.reset(static_cast<float*>(std::malloc(fb_bytes)));
        if (!copy) return at_fail(AT_E_NOMEM, "at_logmel_f32: out of host memory");
        std::memcpy(copy.get(), fb.data(), fb_bytes);
    }
    float* dev = static_cast<float*>(at_ws(ctx, slot, cap_bytes, stream));
    if (!dev) return AT_E_NOMEM;
    // ... then the record describes nothing for as long as the tables on the device are in flux: a call that fails in
    // between leaves a slot the next call rebuilds, never new tables under the old key.
    at_logmel_tables_clear(rec);
    AT_HIP(hipDeviceSynchronize());   // a launch on ANY stream may still be reading the tables about to be replaced
    AT_HIP(hipMemcpy(dev, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice));
    *rec = filled;                    // (nothing between the copy and these two lines can fail)
    rec->user_copy = copy.release();
    *tabs = dev;
    return AT_OK;
}

// The tuned kernel's launch, whatever the clips: this fills the tables, the frames per block, the LDS size and which
// of the two kernels (prefetch or not) applies.
struct Setup512 {
    size_t lds;
    bool pf, fuse_here;
};
static int setup_512(at_ctx* ctx, int sample_rate, int hop, int n_mels, const float* fb_or_null, int fuse_l2norm,
                     hipStream_t stream, LogmelCommon& p, Setup512& su) {
    const at_logmel_tables key{sample_rate, NFFT, n_mels, hop, /* form */ 0};
    const lmt::BlobLayout lay = lmt::blob_layout(TAB_FLOATS, n_mels);
    // (capacity: the worst case, every bin of every filter and its quad padding)
    int rc = at_logmel_resident(ctx, WS_LOGMEL_FB, &ctx->lm_fb, key, (lay.wts + (size_t)(NBIN + 3) * n_mels) * 4, fb_or_null,
                                stream, build_tables_512, &p.tabs);
    if (rc) return rc;
    p.fb_start = reinterpret_cast<const int*>(p.tabs + lay.ints);
    p.fb_len = p.fb_start + n_mels; p.fb_off = p.fb_start + 2 * n_mels;
    p.fb_wts = p.tabs + lay.wts;
    p.fb_nw = ctx->lm_fb.nw; p.fb_quads = ctx->lm_fb.quads;
    p.hop = hop; p.n_mels = n_mels;
    // unit rows are fused for 8 <= n_mels <= 128 (numpy's one-level pairwise sum, eight lanes per frame);
    // other widths get the standalone kernel behind this one, in place
    su.fuse_here = fuse_l2norm && n_mels >= 8 && n_mels <= 128;
    p.fuse_l2norm = su.fuse_here;
    p.bad = fuse_l2norm ? at_row_flag(ctx, stream) : nullptr;
    if (fuse_l2norm && !p.bad) return AT_E_NOMEM;
    // the banded filterbank rides in LDS too unless a dense user filterbank makes it too big
    const size_t fb_ints = lmt::table_ints(n_mels) + p.fb_nw;
    p.fb_lds = fb_ints * 4 <= 14 * 1024;
    // 32 frames per workgroup when two workgroups of that size still share a CU's 160 KiB of LDS
    // (the kernel is latency-bound: one workgroup per CU runs at half the rate), else 16
    su.lds = 0;
    for (p.fpb = 32; p.fpb >= 16; p.fpb -= 16) {
        su.lds = lds_bytes(p.fpb, hop, n_mels, p.fb_lds ? fb_ints : 0);
        if (su.lds <= LDS_TWO_PER_CU || p.fpb == 16) break;
    }
    AT_REQUIRE(su.lds <= 160 * 1024, "at_logmel_f32: n_mels=%d needs %zu bytes of LDS", n_mels, su.lds);
    su.pf = ((p.fpb - 1) * hop + NFFT + 3) / 4 <= PREFETCH_REGS * WG;   // the block's samples fit the prefetch registers
    return AT_OK;
}

static int check_logmel_args(const char* who, at_ctx* ctx, int n_fft, int hop, int n_mels, int layout, int fuse_l2norm) {
    AT_REQUIRE(ctx, "%s: ctx is null", who);
    AT_REQUIRE(n_fft >= 64 && n_fft <= 4096, "%s: n_fft=%d out of range (an even size from 64 to 4096)", who, n_fft);
    AT_REQUIRE((n_fft & 1) == 0,
               "%s: odd n_fft=%d is not supported (torch counts 1 + (L - 1) / hop frames for odd sizes, "
               "at_num_frames has no n_fft argument; use an even size from 64 to 4096)", who, n_fft);
    AT_REQUIRE(hop >= 1 && hop <= n_fft, "%s: hop=%d out of range [1, %d]", who, hop, n_fft);
    AT_REQUIRE(n_mels >= 1 && n_mels <= 1024, "%s: n_mels=%d out of range", who, n_mels);
    AT_REQUIRE(layout == AT_LAYOUT_MEL_MAJOR || layout == AT_LAYOUT_FRAME_MAJOR, "%s: bad layout", who);
    AT_REQUIRE(!fuse_l2norm || layout == AT_LAYOUT_FRAME_MAJOR, "%s: fuse_l2norm needs the frame-major layout", who);
    return AT_OK;
}

// One call of the family, as its entry hands it to the driver.
struct LogmelCall {
    const char* who;
    at_ctx* ctx;
    int sample_rate, n_fft, hop, n_mels;
    const float* fb_or_null;
    float* out;
    int layout, fuse_l2norm;
    bool minmax;            // every clip becomes (spec - min) / (max - min) through the WS_LOGMEL_MINMAX records
    hipStream_t stream;
};
// The clips of a call, as its entry's `prepare` leaves them: the map and its totals (n_frames = 0: nothing to do).
template <typename Clips>
struct ClipSet {
    Clips clips;
    int64_t n_clips, n_frames, n_blocks16, n_blocks32;
};

// Every entry of the family: the checks all share, then the entry's own (`prepare`, which builds the clip map), then
// n_fft = 512 on the tuned kernel or any other size on the general form (logmel_any.hip) over the same map.
// minmax: the records are cleared first; the tuned kernel collects every clip's extremes while a block is still in
// LDS, keyed by the block's clip, every other size is followed by a reduction pass over its output; then the scaling
// pass, which sets the clips' flags where the map has them (the kernel's own unit rows stay off: the rows are scaled
// first).  Last the unit rows the kernel did not fuse, by the stand-alone kernel, in place.  The clips' flags, set from
// the dB values (or the scaled ones), hold for the unit rows: a NaN or Inf in a row makes the row NaN, and a finite
// row stays finite.
template <typename Clips, typename Prepare>
static int logmel_drive(const LogmelCall& c, Prepare prepare) {
    int rc = check_logmel_args(c.who, c.ctx, c.n_fft, c.hop, c.n_mels, c.layout, c.fuse_l2norm);
    if (rc) return rc;
    AT_HIP(hipSetDevice(c.ctx->device));
    ClipSet<Clips> cs{};
    rc = prepare(cs);
    if (rc || cs.n_frames == 0) return rc;
    AT_REQUIRE(cs.clips.wave && c.out, "%s: null pointer", c.who);
    const int frame_major = c.layout == AT_LAYOUT_FRAME_MAJOR;
    MinmaxParams<Clips> mp{};
    long mgrid = 0;
    if (c.minmax) {
        mp.mm = static_cast<unsigned*>(at_ws(c.ctx, WS_LOGMEL_MINMAX, (size_t)cs.n_clips * 16, c.stream));
        if (!mp.mm) return AT_E_NOMEM;
        AT_LAUNCH(minmax_init_kernel, dim3((unsigned)((cs.n_clips + 255) / 256)), dim3(256), 0, c.stream, mp.mm, (long)cs.n_clips);
        mp.x = c.out; mp.total = (long)cs.n_frames * c.n_mels; mp.n_mels = c.n_mels;
        mp.vec = (c.n_mels & 3) == 0 && at_aligned16(c.out);
        mp.clips = cs.clips;
        // one wavefront per MM_CHUNK floats, at most eight workgroups per CU walking the rest
        mgrid = ((mp.total + MM_CHUNK - 1) / MM_CHUNK + 3) / 4;
        if (mgrid > 8L * c.ctx->n_cus) mgrid = 8L * c.ctx->n_cus;
    }
    bool rows_done = false;   // the unit rows came out of the log-mel kernel
    if (c.n_fft != NFFT) {
        rc = at_logmel_any(c.ctx, cs.clips, cs.n_frames, c.sample_rate, c.n_fft, c.hop, c.n_mels, c.fb_or_null, c.out,
                           frame_major, c.stream);
        if (rc) return rc;
        if (c.minmax) AT_LAUNCH(minmax_extremes_kernel<Clips>, dim3((unsigned)mgrid), dim3(256), 0, c.stream, mp);
    } else {
        LogmelParams<Clips> p;
        Setup512 su;
        rc = setup_512(c.ctx, c.sample_rate, c.hop, c.n_mels, c.fb_or_null, c.minmax ? 0 : c.fuse_l2norm, c.stream, p, su);
        if (rc) return rc;
        p.clips = cs.clips;
        p.out = c.out; p.frame_major = frame_major;
        p.minmax = mp.mm;
        p.n_blocks = (long)(p.fpb == 32 ? cs.n_blocks32 : cs.n_blocks16);
        AT_RAISE_LDS(c.ctx, (logmel_kernel<true, Clips>), su.lds);
        AT_RAISE_LDS(c.ctx, (logmel_kernel<false, Clips>), su.lds);
        // persistent workgroups: two per CU (what the LDS footprint allows), each walking a strided share
        // of the blocks with its window / twiddle tables in registers
        long grid = 2L * c.ctx->n_cus;
        if (grid > p.n_blocks) grid = p.n_blocks;
        if (su.pf) AT_LAUNCH((logmel_kernel<true, Clips>), dim3((unsigned)grid), dim3(WG), su.lds, c.stream, p);
        else AT_LAUNCH((logmel_kernel<false, Clips>), dim3((unsigned)grid), dim3(WG), su.lds, c.stream, p);
        rows_done = su.fuse_here;
    }
    if (c.minmax) AT_LAUNCH(minmax_scale_pieces_kernel<Clips>, dim3((unsigned)mgrid), dim3(256), 0, c.stream, mp);
    if (c.fuse_l2norm && !rows_done) {
        int* flag = at_row_flag(c.ctx, c.stream);
        if (!flag) return AT_E_NOMEM;
        rc = at_l2norm_rows_flagged(c.ctx, c.out, cs.n_frames, c.n_mels, c.out, flag, c.stream);
    }
    return rc;
}

// The uniform entries: n_clips rows of L samples.  minmax: n_fft = 512 only (at_logmel_minmax_f32).
static int logmel_uniform(at_ctx* ctx, const float* wave, int64_t n_clips, int64_t L, int64_t wave_stride, int sample_rate,
                          int n_fft, int hop, int n_mels, const float* fb_or_null, float* out, int layout, int fuse_l2norm,
                          bool minmax, hipStream_t stream) {
    const LogmelCall c{"at_logmel_f32", ctx, sample_rate, n_fft, hop, n_mels, fb_or_null, out, layout, fuse_l2norm, minmax, stream};
    return logmel_drive<lmc::UniformClips>(c, [&](ClipSet<lmc::UniformClips>& cs) -> int {
        AT_REQUIRE(n_clips >= 0 && n_clips <= 65535 * 1024L, "at_logmel_f32: n_clips out of range");
        AT_REQUIRE(L > n_fft / 2, "at_logmel_f32: clip length %lld must exceed n_fft/2 (reflect padding)", (long long)L);
        AT_REQUIRE(wave_stride >= L, "at_logmel_f32: wave_stride < L");
        if (n_clips == 0) return AT_OK;
        const int64_t T = at_num_frames(L, hop);
        AT_REQUIRE(T < (1LL << 31), "at_logmel_f32: too many frames per clip");
        cs.clips = lmc::UniformClips{wave, L, wave_stride, (int)T};
        cs.n_clips = n_clips;
        cs.n_frames = n_clips * T;
        cs.n_blocks16 = (T + 15) / 16 * n_clips;
        cs.n_blocks32 = (T + 31) / 32 * n_clips;
        return AT_OK;
    });
}

// at_logmel_f32 for the clips of an at_frontend_plan_host plan, one launch (include/audio_tokens_amd.h): the same
// kernels over the same tables as the uniform call, over the plan's map.
static int logmel_ragged(const char* who, at_ctx* ctx, const float* mono, const at_frontend_clip* plan_dev, int64_t n_clips,
                         const at_frontend_totals* totals, int sample_rate, int n_fft, int hop, int n_mels,
                         const float* fb_or_null, float* out, int layout, int fuse_l2norm, int32_t* bad, bool minmax,
                         hipStream_t stream) {
    const LogmelCall c{who, ctx, sample_rate, n_fft, hop, n_mels, fb_or_null, out, layout, fuse_l2norm, minmax, stream};
    return logmel_drive<lmc::PlanClips>(c, [&](ClipSet<lmc::PlanClips>& cs) -> int {
        AT_REQUIRE(n_clips >= 0 && n_clips < (1LL << 31), "%s: n_clips out of range", who);
        if (n_clips == 0) return AT_OK;
        AT_REQUIRE(totals && plan_dev && bad, "%s: null pointer", who);
        AT_REQUIRE(totals->n_frames >= 0 && totals->n_blocks16 >= 0 && totals->n_blocks32 >= 0 &&
                       totals->n_blocks32 <= totals->n_blocks16 && totals->n_blocks16 <= totals->n_frames,
                   "%s: bad totals", who);
        AT_HIP(hipMemsetAsync(bad, 0, (size_t)n_clips * sizeof(int32_t), stream));
        cs.clips = lmc::PlanClips{mono, plan_dev, (long)n_clips, bad};
        cs.n_clips = n_clips;
        cs.n_frames = totals->n_frames;   // (0: every clip too short)
        cs.n_blocks16 = totals->n_blocks16;
        cs.n_blocks32 = totals->n_blocks32;
        return AT_OK;
    });
}

extern "C" int at_logmel_ragged_f32(at_ctx* ctx, const float* mono, const at_frontend_clip* plan_dev, int64_t n_clips,
                                    const at_frontend_totals* totals, int sample_rate, int n_fft, int hop, int n_mels,
                                    const float* fb_or_null, float* out, int layout, int fuse_l2norm, int32_t* bad,
                                    void* stream_) {
    return logmel_ragged("at_logmel_ragged_f32", ctx, mono, plan_dev, n_clips, totals, sample_rate, n_fft, hop, n_mels,
                         fb_or_null, out, layout, fuse_l2norm, bad, false, (hipStream_t)stream_);
}

// every clip becomes (spec - min) / (max - min) before the unit rows, if any
extern "C" int at_logmel_ragged_minmax_f32(at_ctx* ctx, const float* mono, const at_frontend_clip* plan_dev, int64_t n_clips,
                                           const at_frontend_totals* totals, int sample_rate, int n_fft, int hop, int n_mels,
                                           const float* fb_or_null, float* out, int layout, int fuse_l2norm, int32_t* bad,
                                           void* stream_) {
    return logmel_ragged("at_logmel_ragged_minmax_f32", ctx, mono, plan_dev, n_clips, totals, sample_rate, n_fft, hop,
                         n_mels, fb_or_null, out, layout, fuse_l2norm, bad, true, (hipStream_t)stream_);
}

extern "C" int at_logmel_f32(at_ctx* ctx, const float* wave, int64_t n_clips, int64_t L,
                             int64_t wave_stride, int sample_rate, int n_fft, int hop, int n_mels,
                             const float* fb_or_null, float* out, int layout, int fuse_l2norm,
                             void* stream_) {
    return logmel_uniform(ctx, wave, n_clips, L, wave_stride, sample_rate, n_fft, hop, n_mels, fb_or_null, out, layout,
                          fuse_l2norm, false, (hipStream_t)stream_);
}

// MelSpectrogram + AmplitudeToDB + normalize_spectrogram (processors/spectrogram_generator.py:123-131 with
// config.normalize = True): the log-mel kernel collects every clip's smallest and largest dB value while the block it
// has just computed is still in LDS, so the scaling is ONE pass over the spectrogram (8 B per value) instead of a
// reduction pass plus a scaling pass (12 B).  Other n_fft than 512: the general log-mel kernel, then the two-pass form
// that needs no scratch (l2norm.hip).
extern "C" int at_logmel_minmax_f32(at_ctx* ctx, const float* wave, int64_t n_clips, int64_t L, int64_t wave_stride,
                                    int sample_rate, int n_fft, int hop, int n_mels, const float* fb_or_null, float* out,
                                    int layout, void* stream_) {
    AT_REQUIRE(ctx, "at_logmel_minmax_f32: ctx is null");
    if (n_clips == 0) return AT_OK;
    const bool fused = n_fft == NFFT;
    AT_REQUIRE(!fused || n_clips <= 65535, "at_logmel_minmax_f32: at most 65535 clips per call");
    const int rc = logmel_uniform(ctx, wave, n_clips, L, wave_stride, sample_rate, n_fft, hop, n_mels, fb_or_null, out, layout,
                                  0, fused, (hipStream_t)stream_);
    if (rc || fused) return rc;
    // (logmel_uniform has checked every argument by now)
    return at_minmax_scale_clips_f32(ctx, out, n_clips, at_num_frames(L, hop) * n_mels, stream_);
}
