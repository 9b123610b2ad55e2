// resample.hip -- torchaudio.transforms.Resample(orig_freq, new_freq) on gfx950 (at_resample_f32).
//
// Replaces SpectrogramGenerator.resample (processors/spectrogram_generator.py:117-121 of
// danavery/audio-tokens): torchaudio 2.4.1 Resample with its defaults -- resampling_method
// "sinc_interp_hann", lowpass_filter_width = 6, rolloff = 0.99 -- i.e. a polyphase FIR: with
// orig/new reduced by their gcd, output sample i*new + j is the dot product of the j-th filter
// (2*width + orig taps) with the input window starting at i*orig - width (zero padded).
// HBM-bound in principle (4 B in + 4*new/orig B out per input sample); every input sample is
// re-read new*K/orig times from L1/L2.
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "at_internal.h"

namespace {

constexpr int WG = 256;

// Where a kernel's input samples come from: a mono row, or the mean of a stereo pair -- (l + r) * 0.5f, the bits of
// torch.mean over two rows (convert_to_mono, processors/spectrogram_generator.py:105-108).  Index in [0, L).
struct MonoSrc {
    const float* w;
    __device__ __forceinline__ float operator()(long s) const { return w[s]; }
};
struct StereoSrc {
    const float* l;
    const float* r;
    __device__ __forceinline__ float operator()(long s) const { return (l[s] + r[s]) * 0.5f; }
};

// output sample o of one clip: the ascending-k fma chain over the taps of its phase
template <typename Src>
__device__ __forceinline__ float resample_point(const Src& w, long L, const float* __restrict__ taps, int orig, int nw, int K,
                                                int width, long o) {
    const long i = o / nw;
    const int j = (int)(o - i * nw);
    const float* t = taps + j;  // device taps are stored [K][new]: consecutive lanes, consecutive phases
    const long s0 = i * orig - width;
    float acc = 0.0f;
    for (int k = 0; k < K; k++) {
        const long s = s0 + k;
        const float v = (s >= 0 && s < L) ? w(s) : 0.0f;
        acc = __builtin_fmaf(v, t[(size_t)k * nw], acc);
    }
    return acc;
}

__global__ void __launch_bounds__(WG) resample_kernel(const float* __restrict__ wave, long n_clips, long L,
                                                      long wave_stride, const float* __restrict__ taps, int orig,
                                                      int nw, int K, int width, long out_len, long out_stride,
                                                      float* __restrict__ out) {
    const long o = (long)blockIdx.x * WG + threadIdx.x;
    const long clip = blockIdx.y;
    if (o >= out_len) return;
    out[clip * out_stride + o] = resample_point(MonoSrc{wave + clip * wave_stride}, L, taps, orig, nw, K, width, o);
}

// Tiled variant: the input span of TI consecutive i-steps is staged in LDS once and every thread
// keeps RI accumulators for one phase j, so a tap fetched from L1 feeds RI FMAs.  When the number
// of phases is large the RI steps of a thread are adjacent (all lanes of a wave then read the same
// LDS word: a broadcast); when it is small (44.1 kHz -> 22.05 kHz has ONE phase) they are
// interleaved so that consecutive lanes read consecutive steps.  The accumulation order is the
// same ascending-k fma chain as resample_kernel, so both produce identical bits.
// One tile: the i-steps [i0, i0 + TI) of the clip `w` (L samples, L > 0), written to o[0 .. out_len).
template <int RI, typename Src>
__device__ __forceinline__ void resample_tile(const Src& w, long L, const float* __restrict__ taps, int orig, int nw, int K,
                                              int width, int TI, int interleave, long i0, long out_len,
                                              float* __restrict__ o, float* seg) {
    const int span = (TI - 1) * orig + K;
    const long s_base = i0 * orig - width;
    // eight independent (clamped, then masked) loads in flight per thread: the staging is otherwise
    // one exposed HBM latency per 1 KiB
    for (int t0 = threadIdx.x; t0 < span; t0 += WG * 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const long s = s_base + t0 + u * WG;
            const long sc = s < 0 ? 0 : (s >= L ? L - 1 : s);
            v[u] = w(sc);
            if (s != sc) v[u] = 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (t0 + u * WG < span) seg[t0 + u * WG] = v[u];
    }
    __syncthreads();
    const int nblk = TI / RI;
    const int ntask = nw * nblk;
    for (int q = threadIdx.x; q < ntask; q += WG) {
        const int ib = q / nw;
        const int j = q - ib * nw;
        int li[RI];
#pragma unroll
        for (int r = 0; r < RI; r++) li[r] = interleave ? r * nblk + ib : ib * RI + r;
        float acc[RI];
#pragma unroll
        for (int r = 0; r < RI; r++) acc[r] = 0.0f;
        const float* tp = taps + j;
#pragma unroll 4
        for (int k = 0; k < K; k++) {
            const float t = tp[(size_t)k * nw];
#pragma unroll
            for (int r = 0; r < RI; r++) acc[r] = __builtin_fmaf(seg[li[r] * orig + k], t, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < RI; r++) {
            const long oi = (i0 + li[r]) * nw + j;
            if (oi < out_len) o[oi] = acc[r];
        }
    }
}

template <int RI>
__global__ void __launch_bounds__(WG) resample_tiled_kernel(const float* __restrict__ wave, long L, long wave_stride,
                                                            const float* __restrict__ taps, int orig, int nw, int K,
                                                            int width, int TI, int interleave, long out_len,
                                                            long out_stride, float* __restrict__ out) {
    extern __shared__ float seg[];
    const long clip = blockIdx.y;
    resample_tile<RI>(MonoSrc{wave + clip * wave_stride}, L, taps, orig, nw, K, width, TI, interleave, (long)blockIdx.x * TI,
                      out_len, out + clip * out_stride, seg);
}

// ---- the ragged form: all clips of one rate-pair group of an at_frontend_plan_host plan in one launch ---------------
// Workgroup b of the launch belongs to the clip whose rs_first_block is the last one <= b among the group's clips
// (order[0 .. count), prefix sums ascending; a clip without blocks shares its prefix with the clip behind it and is
// never found), and is that clip's block b - rs_first_block: out_per_block output samples.
struct RaggedRs {
    const float* in;
    const at_frontend_clip* plan;
    const int32_t* order;   // the group's slice
    long count;
    float* mono;
    const float* taps;
    int orig, nw, K, width, TI, interleave;
    long out_per_block;
};

template <int MODE, bool STEREO>
__device__ __forceinline__ void ragged_rs_block(const RaggedRs& p, const at_frontend_clip& c, long b, float* seg) {
    const float* w = p.in + c.in_offset;
    using Src = typename std::conditional<STEREO, StereoSrc, MonoSrc>::type;
    Src src;
    if constexpr (STEREO) src = StereoSrc{w, w + c.in_row_stride};
    else src = MonoSrc{w};
    float* o = p.mono + c.mono_offset;
    if constexpr (MODE == AT_FRONTEND_TILED) {
        // (a tile no longer than what is left of the clip, as at_resample_f32 sizes its tiles: which thread computes
        // which sample changes, no sample's arithmetic does)
        const long i0 = b * p.TI, left = (c.out_length + p.nw - 1) / p.nw - i0;
        const long ti = left < p.TI ? (left + AT_RS_RI - 1) / AT_RS_RI * AT_RS_RI : p.TI;
        resample_tile<AT_RS_RI>(src, c.in_length, p.taps, p.orig, p.nw, p.K, p.width, (int)ti, p.interleave, i0, c.out_length, o,
                                seg);
    } else {
        const long e1 = (b + 1) * p.out_per_block < c.out_length ? (b + 1) * p.out_per_block : (long)c.out_length;
        for (long e = b * p.out_per_block + threadIdx.x; e < e1; e += WG) {
            if constexpr (MODE == AT_FRONTEND_SIMPLE) o[e] = resample_point(src, c.in_length, p.taps, p.orig, p.nw, p.K, p.width, e);
            else o[e] = src(e);
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(WG) mix_resample_ragged_kernel(RaggedRs p) {
    extern __shared__ float seg[];
    const long b = blockIdx.x;
    long lo = 0, hi = p.count;   // the last j with plan[order[j]].rs_first_block <= b
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (p.plan[p.order[mid]].rs_first_block <= b) lo = mid;
        else hi = mid;
    }
    const at_frontend_clip c = p.plan[p.order[lo]];
    if (c.channels == 2) ragged_rs_block<MODE, true>(p, c, b - c.rs_first_block, seg);
    else ragged_rs_block<MODE, false>(p, c, b - c.rs_first_block, seg);
}

// The polyphase taps of (orig_freq, new_freq), transposed to [K][new], resident in workspace `slot`; key[2] says what
// the slot holds.
int resident_taps(at_ctx* ctx, int slot, int* key, int orig_freq, int new_freq, hipStream_t stream, const float** taps_out) {
    if (!(key[0] == orig_freq && key[1] == new_freq && ctx->ws[slot])) {
        int orig = 0, nw = 0, width = 0;
        int rc = at_resample_taps_host(orig_freq, new_freq, &orig, &nw, &width, nullptr, 0);
        if (rc) return rc;
        const int K = 2 * width + orig;
        std::vector<float> taps((size_t)nw * K);
        rc = at_resample_taps_host(orig_freq, new_freq, &orig, &nw, &width, taps.data(), (int64_t)taps.size());
        if (rc) return rc;
        std::vector<float> tr((size_t)nw * K);
        for (int j = 0; j < nw; j++)
            for (int k = 0; k < K; k++) tr[(size_t)k * nw + j] = taps[(size_t)j * K + k];
        key[0] = key[1] = 0;
        float* dev = static_cast<float*>(at_ws(ctx, slot, tr.size() * sizeof(float), stream));
        if (!dev) return AT_E_NOMEM;
        AT_HIP(hipStreamSynchronize(stream));
        AT_HIP(hipMemcpy(dev, tr.data(), tr.size() * sizeof(float), hipMemcpyHostToDevice));
        key[0] = orig_freq; key[1] = new_freq;
    }
    *taps_out = static_cast<const float*>(ctx->ws[slot]);
    return AT_OK;
}

}  // namespace

extern "C" {

// torchaudio.functional._get_sinc_resample_kernel (sinc_interp_hann), evaluated in double and
// rounded to float as torchaudio does.  taps_host: [new][2*width + orig]; returns width via *width.
int at_resample_taps_host(int orig_freq, int new_freq, int* orig_out, int* new_out, int* width_out,
                          float* taps_host, int64_t taps_capacity) {
    AT_REQUIRE(orig_freq > 0 && new_freq > 0 && orig_out && new_out && width_out, "at_resample_taps_host: bad arguments");
    int a = orig_freq, b = new_freq;
    while (b) { const int t = a % b; a = b; b = t; }
    const int g = a;
    const int orig = orig_freq / g, nw = new_freq / g;
    const double lowpass_filter_width = 6.0, rolloff = 0.99;
    const double base_freq = std::fmin((double)orig, (double)nw) * rolloff;
    const int width = (int)std::ceil(lowpass_filter_width * orig / base_freq);
    const int K = 2 * width + orig;
    *orig_out = orig; *new_out = nw; *width_out = width;
    if (!taps_host) return AT_OK;  // size query
    AT_REQUIRE(taps_capacity >= (int64_t)nw * K, "at_resample_taps_host: taps buffer too small");
    const double scale = base_freq / orig;
    for (int j = 0; j < nw; j++) {
        for (int k = 0; k < K; k++) {
            double t = (double)(-j) / nw + (double)(k - width) / orig;
            t *= base_freq;
            if (t < -lowpass_filter_width) t = -lowpass_filter_width;
            if (t > lowpass_filter_width) t = lowpass_filter_width;
            const double c = std::cos(t * M_PI / lowpass_filter_width / 2.0);
            const double window = c * c;
            t *= M_PI;
            const double sinc = t == 0.0 ? 1.0 : std::sin(t) / t;
            taps_host[(size_t)j * K + k] = (float)(sinc * window * scale);
        }
    }
    return AT_OK;
}

int64_t at_resample_length(int64_t L, int orig_freq, int new_freq) {
    int a = orig_freq, b = new_freq;
    while (b) { const int t = a % b; a = b; b = t; }
    const int64_t orig = orig_freq / a, nw = new_freq / a;
    return (nw * L + orig - 1) / orig;  // ceil(new * length / orig)
}

int at_resample_f32(at_ctx* ctx, const float* wave, int64_t n_clips, int64_t L, int64_t wave_stride,
                    int orig_freq, int new_freq, float* out, int64_t out_stride, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx && orig_freq > 0 && new_freq > 0 && n_clips >= 0 && L > 0, "at_resample_f32: bad arguments");
    if (n_clips == 0) return AT_OK;
    AT_REQUIRE(wave && out && wave_stride >= L && n_clips <= 65535, "at_resample_f32: bad arguments");
    AT_HIP(hipSetDevice(ctx->device));
    int orig = 0, nw = 0, width = 0;
    int rc = at_resample_taps_host(orig_freq, new_freq, &orig, &nw, &width, nullptr, 0);
    if (rc) return rc;
    const int K = 2 * width + orig;
    const int64_t out_len = at_resample_length(L, orig_freq, new_freq);
    AT_REQUIRE(out_stride >= out_len, "at_resample_f32: out_stride < output length %lld", (long long)out_len);
    const float* taps = nullptr;
    int key[2] = {ctx->rs_orig, ctx->rs_new};
    rc = resident_taps(ctx, WS_RESAMPLE_TAPS, key, orig_freq, new_freq, stream, &taps);
    ctx->rs_orig = key[0]; ctx->rs_new = key[1];
    if (rc) return rc;
    constexpr int RI = AT_RS_RI;
    constexpr int kSegFloats = AT_RS_SEG_FLOATS;  // 32 KiB of LDS per workgroup
    const bool force_simple = ctx->dbg.resample_simple != 0;  // test switch
    const long fit = ((long)kSegFloats - K) / orig + 1;  // i-steps whose input span fits the segment
    if (fit >= RI && !force_simple) {
        const long n_i = (out_len + nw - 1) / nw;
        long TI = fit - fit % RI;
        const long cap = ((n_i + RI - 1) / RI) * RI;  // no point in tiles longer than the clip
        if (TI > cap) TI = cap;
        const size_t lds = sizeof(float) * (size_t)((TI - 1) * orig + K);
        AT_LAUNCH(resample_tiled_kernel<RI>, dim3((unsigned)((n_i + TI - 1) / TI), (unsigned)n_clips),
                           dim3(WG), lds, stream, wave, (long)L, (long)wave_stride, taps, orig, nw, K, width, (int)TI,
                           nw < 32 ? 1 : 0, (long)out_len, (long)out_stride, out);
    } else {
        AT_LAUNCH(resample_kernel, dim3((unsigned)((out_len + WG - 1) / WG), (unsigned)n_clips), dim3(WG),
                           0, stream, wave, (long)n_clips, (long)L, (long)wave_stride, taps, orig, nw, K, width,
                           (long)out_len, (long)out_stride, out);
    }
    return AT_OK;
}

// One rate-pair group of an at_frontend_plan_host plan (include/audio_tokens_amd.h): mono mix and resampler for all
// of its clips in one launch.  The taps of up to four rate pairs stay resident, so a dataset that mixes 44.1 kHz and
// 48 kHz files builds each set once.
int at_mix_resample_ragged_f32(at_ctx* ctx, const float* in, const at_frontend_clip* plan_dev, const int32_t* order_dev,
                               const at_frontend_group* group, float* mono, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx && group, "at_mix_resample_ragged_f32: null pointer");
    const at_frontend_group& G = *group;
    AT_REQUIRE(G.count >= 0 && G.first >= 0 && G.n_blocks >= 0 && G.n_blocks < (1LL << 31),
               "at_mix_resample_ragged_f32: bad group record");
    if (G.count == 0 || G.n_blocks == 0) return AT_OK;
    AT_REQUIRE(in && plan_dev && order_dev && mono, "at_mix_resample_ragged_f32: null pointer");
    AT_REQUIRE(G.orig > 0 && G.nw > 0 && G.out_per_block > 0, "at_mix_resample_ragged_f32: bad group record");
    AT_HIP(hipSetDevice(ctx->device));
    RaggedRs p{};
    p.in = in; p.plan = plan_dev; p.order = order_dev + G.first; p.count = (long)G.count; p.mono = mono;
    p.orig = G.orig; p.nw = G.nw; p.out_per_block = (long)G.out_per_block;
    const dim3 grid((unsigned)G.n_blocks), block(WG);
    if (G.mode == AT_FRONTEND_COPY) {
        AT_REQUIRE(G.orig == G.nw, "at_mix_resample_ragged_f32: a group without a filter must have equal rates");
        AT_LAUNCH(mix_resample_ragged_kernel<AT_FRONTEND_COPY>, grid, block, 0, stream, p);
        return AT_OK;
    }
    // what the plan says about the filter is checked against the filter itself: the kernels trust these numbers
    int orig = 0, nw = 0, width = 0;
    int rc = at_resample_taps_host(G.orig_freq, G.new_freq, &orig, &nw, &width, nullptr, 0);
    if (rc) return rc;
    AT_REQUIRE(orig == G.orig && nw == G.nw && width == G.width && G.K == 2 * width + orig,
               "at_mix_resample_ragged_f32: the group record does not describe the filter of %d -> %d", G.orig_freq, G.new_freq);
    int slot = -1;
    for (int i = 0; i < 4; i++)
        if (ctx->rg_taps[i][0] == G.orig && ctx->rg_taps[i][1] == G.nw && ctx->ws[WS_RAGGED_TAPS0 + i]) slot = i;
    if (slot < 0) slot = ctx->rg_next++ & 3;
    rc = resident_taps(ctx, WS_RAGGED_TAPS0 + slot, ctx->rg_taps[slot], G.orig, G.nw, stream, &p.taps);   // (reduced pair: same taps)
    if (rc) return rc;
    p.K = G.K; p.width = G.width;
    if (G.mode == AT_FRONTEND_TILED) {
        AT_REQUIRE(G.TI >= AT_RS_RI && G.TI % AT_RS_RI == 0 && (long)(G.TI - 1) * G.orig + G.K <= AT_RS_SEG_FLOATS &&
                       G.out_per_block == (int64_t)G.TI * G.nw,
                   "at_mix_resample_ragged_f32: bad tile size in the group record");
        p.TI = G.TI; p.interleave = G.nw < 32 ? 1 : 0;
        const size_t lds = sizeof(float) * (size_t)((G.TI - 1) * G.orig + G.K);
        AT_LAUNCH(mix_resample_ragged_kernel<AT_FRONTEND_TILED>, grid, block, lds, stream, p);
    } else {
        AT_REQUIRE(G.mode == AT_FRONTEND_SIMPLE, "at_mix_resample_ragged_f32: bad mode");
        AT_LAUNCH(mix_resample_ragged_kernel<AT_FRONTEND_SIMPLE>, grid, block, 0, stream, p);
    }
    return AT_OK;
}

}  // extern "C"
