// logmel_any.hip -- at_logmel_f32 for every even n_fft other than 512 (64 .. 4096).
//
// The reference exposes n_fft / hop_length as configuration (audio_tokens_config.py:39-40; its README
// documents 1024 / 512) and hands them to torchaudio's MelSpectrogram (processors/spectrogram_generator.py:28-33).
// The tuned kernel (logmel.hip) is built around the code default, n_fft = 512 -- two 16-point stages in registers.
// This file is the general form: one wavefront per frame, the M = n_fft/2-point complex FFT of z[m] = x[2m] + i x[2m+1]
// as Stockham passes of radix 8 (then 4 or 2 for what is left of log2 M) with the butterflies in registers: three
// passes and two trips through LDS at n_fft = 1024 (round 2 did nine radix-2 stages, each a trip through LDS, with
// window and twiddles read from global memory); the first pass takes the windowed samples straight from global
// memory, twiddle and window tables sit in LDS.  Then the same even/odd untangling to the M + 1 power bins, the banded
// mel dot products, 10 log10.  Same arithmetic contract as the tuned kernel (fp32 throughout, |X|^2 as re^2 + im^2,
// clamp at 1e-10), same tolerance against the CPU restatement (tests/test_gpu_ops.py::test_logmel_other_nfft).
// Which clip a frame belongs to is the clip map's business (logmel_clips.h): every kernel here is a template on it.
// The even sizes that are not powers of two (400, 480, 1000, ...) take logmel_mixed_kernel further down: run-time
// radices from {8, 4, 2, 3, 5, 7} where M has no larger prime factor, Bluestein's chirp transform elsewhere
// (logmel_mixed_core.h; tests/test_gpu_logmel_nfft.py).
#include <cmath>
#include <vector>

#include "at_internal.h"
#include "logmel_clips.h"
#include "logmel_mixed_core.h"
#include "logmel_tables.h"

namespace {

using namespace lmx;

constexpr int WG = 256;

struct AnyCommon {
    int n_fft, log2m, hop, n_mels;
    long n_frames;           // of all clips
    const float* win;        // n_fft
    const float* twm;        // M x (cos, -sin) of 2*pi*q/M
    const float* twn;        // M x (cos, -sin) of 2*pi*k/n_fft
    const int* fb_start;     // [n_mels] first bin / number of bins / offset into fb_wts
    const int* fb_len;
    const int* fb_off;
    const float* fb_wts;
    float* out;
    int frame_major;
};
// Clips: the map from an output frame to its clip (logmel_clips.h)
template <typename Clips>
struct AnyParams : AnyCommon {
    Clips clips;
};
using lmc::ClipAt;

// One Stockham pass of radix R over M points held by one wavefront: butterfly j (of M/R) takes the inputs
// j + t*M/R, multiplies input t by W_(NS*R)^(k*t) with k = j mod NS (NS = product of the radices before this pass),
// and leaves the R outputs at (j - k)*R + k + t*NS.  Natural order in, natural order out after the last pass.
// In place: a wavefront's LDS instructions execute in order, and every lane has read all its inputs into registers
// before the first store of the pass is issued (the wave barriers keep the compiler from mixing the two).
template <int M, int R, int NS, bool FIRST, typename Load>
__device__ __forceinline__ void fft_pass(int lane, float* z, const float* tw, Load load) {
    constexpr int NB = M / R;
    constexpr int PER = (NB + 63) / 64;
    cx v[PER][R];
#pragma unroll
    for (int b = 0; b < PER; b++) {
        const int j = lane + 64 * b;
        if (NB >= 64 * (b + 1) || j < NB) {
#pragma unroll
            for (int t = 0; t < R; t++) {
                if constexpr (FIRST) v[b][t] = load(j + t * NB);
                else v[b][t] = {z[2 * (j + t * NB)], z[2 * (j + t * NB) + 1]};
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int b = 0; b < PER; b++) {
        const int j = lane + 64 * b;
        if (NB >= 64 * (b + 1) || j < NB) {
            const int k = j & (NS - 1);
            if constexpr (NS > 1) {
#pragma unroll
                for (int t = 1; t < R; t++) {
                    const int q = k * t * (M / (NS * R));
                    v[b][t] = cmul(v[b][t], {tw[2 * q], tw[2 * q + 1]});
                }
            }
            dftR<R>(v[b]);
            const int j0 = (j - k) * R + k;
#pragma unroll
            for (int t = 0; t < R; t++) {
                z[2 * (j0 + t * NS)] = v[b][t].re;
                z[2 * (j0 + t * NS) + 1] = v[b][t].im;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// radix 8 while three bits are left, then 4 or 2
template <int M, int NS, bool FIRST, typename Load>
__device__ __forceinline__ void fft_passes(int lane, float* z, const float* tw, Load load) {
    if constexpr (NS < M) {
        constexpr int left = M / NS;
        constexpr int R = left >= 8 ? 8 : left;
        fft_pass<M, R, NS, FIRST>(lane, z, tw, load);
        fft_passes<M, NS * R, false>(lane, z, tw, load);
    }
}

// ---- what the power-of-two kernel and the mixed-radix / Bluestein kernel share --------------------------------------
// One frame's source: complex point m = (x[2m], x[2m+1]) of the windowed frame (torch: frames * window, fp32), with
// center=True's n_fft/2 samples of reflection on each side.
struct FrameSrc {
    const float* w;     // the clip
    const float* win;   // n_fft window values
    long s0, L;
    bool inner;         // no reflection anywhere in this frame
    __device__ __forceinline__ FrameSrc(const AnyCommon& p, const ClipAt& f, const float* win_)
        : w(f.w), win(win_), s0((long)f.t * p.hop - p.n_fft / 2), L(f.L) {
        inner = s0 >= 0 && s0 + p.n_fft <= L;
    }
    __device__ __forceinline__ cx operator()(int m) const {
        float v[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            long q = s0 + 2 * m + e;
            if (!inner) q = reflect_index(q, L);
            v[e] = w[q] * win[2 * m + e];
        }
        return {v[0], v[1]};
    }
};

struct WaveBarrier {
    __device__ __forceinline__ void operator()() const { __builtin_amdgcn_wave_barrier(); }
};

// Z (M complex points, natural order) -> the M + 1 power bins
__device__ __forceinline__ void untangle_frame(int lane, int M, const float* z, const float* twn, float* pw) {
    untangle_lanes(Lanes{lane, lane + 1}, M, z, twn, pw, WaveBarrier{});
}

// banded mel dot products, 10 log10, store in either layout
template <typename Clips>
__device__ __forceinline__ void mel_db_store(int lane, const AnyParams<Clips>& p, const float* pw, long g, const ClipAt& f) {
    int flagged = 0;
    for (int m = lane; m < p.n_mels; m += 64) {
        const float* wt = p.fb_wts + p.fb_off[m];
        const int st = p.fb_start[m], ln = p.fb_len[m];
        float acc = 0.0f;
        for (int q = 0; q < ln; q++) acc = __builtin_fmaf(pw[st + q], wt[q], acc);
        const float db = !(acc <= 1e-10f) ? 10.0f * log10f(acc) : -100.0f;   // (a NaN power stays NaN, as torch.clamp leaves it)
        if constexpr (Clips::has_flags) flagged |= !(__builtin_fabsf(db) < __builtin_inff());
        if (p.frame_major) p.out[g * p.n_mels + m] = db;
        else p.out[f.base * p.n_mels + (long)m * f.T + f.t] = db;
    }
    if constexpr (Clips::has_flags)
        if (flagged) p.clips.flags[f.clip] = 1;   // (every writer stores the same value)
    __builtin_amdgcn_wave_barrier();   // the next frame overwrites the buffers
}

template <int LOG2M, typename Clips>
__global__ void __launch_bounds__(WG) logmel_any_kernel(AnyParams<Clips> p) {
    constexpr int M = 1 << LOG2M, N = 2 * M;
    extern __shared__ __attribute__((aligned(16))) float sm[];   // W_M (2M) | W_N (2M) | window (N) | per wave: z (N) + power (M + 4)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* tw = sm;
    float* twn = sm + 2 * M;
    float* win = sm + 4 * M;
    for (int i = threadIdx.x; i < 2 * M; i += WG) {
        tw[i] = p.twm[i];
        twn[i] = p.twn[i];
        win[i] = p.win[i];
    }
    __syncthreads();
    float* z = sm + 6 * M + (size_t)wave * (N + M + 4);
    float* pw = z + N;
    for (long g = (long)blockIdx.x * (WG / 64) + wave; g < p.n_frames; g += (long)gridDim.x * (WG / 64)) {
        const ClipAt f = p.clips.by_frame(g);
        const FrameSrc load(p, f, win);
        fft_passes<M, 1, true>(lane, z, tw, load);
        untangle_frame(lane, M, z, twn, pw);
        mel_db_store(lane, p, pw, g, f);
    }
}

// Every even n_fft that is not a power of two (logmel_mixed_core.h).  BLUE = false: form 1, the M-point transform as
// mixed-radix Stockham passes.  BLUE = true: form 2, Bluestein's chirp transform with two P-point power-of-two
// transforms.  A pass reads one of the wave's two buffers and writes the other (the first pass of a transform reads
// its input where it lies: global memory, or the product with the filter's transform), so a lane never has to hold
// more than one butterfly; a wavefront's LDS instructions execute in order and the wave barriers keep the compiler
// from moving an access across a pass boundary.  The window stays in global memory (read once per sample, coalesced):
// two P-point buffers per wave are what the LDS is spent on.  blockDim.x / 64 waves per workgroup (1 .. 4, by LDS).
template <typename Clips>
struct MixedParams {
    AnyParams<Clips> a;
    int P, npass;
    unsigned long long packed;   // lmx::Plan::packed
    const float* twp;            // P x (cos, -sin) of 2*pi*q/P
    const float* chirp;          // form 2: M x w[n]
    const float* bhat;           // form 2: P x transform of the chirp filter, / P
};

// (__launch_bounds__(WG) is the upper bound: the launch uses 64 .. 256 threads, launch_mixed)
template <bool BLUE, typename Clips>
__global__ void __launch_bounds__(WG) logmel_mixed_kernel(MixedParams<Clips> p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];   // W_P (2P) | W_N (2M) | per wave: two buffers of 2P
    const int M = p.a.n_fft / 2, P = p.P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    float* tw = sm;
    float* twn = sm + 2 * P;
    for (int i = threadIdx.x; i < 2 * P; i += blockDim.x) tw[i] = p.twp[i];
    for (int i = threadIdx.x; i < 2 * M; i += blockDim.x) twn[i] = p.a.twn[i];
    __syncthreads();
    float* buf = sm + 2 * P + 2 * M + (size_t)wave * 4 * P;
    for (long g = (long)blockIdx.x * nw + wave; g < p.a.n_frames; g += (long)gridDim.x * nw) {
        const ClipAt f = p.a.clips.by_frame(g);
        const FrameSrc src(p.a, f, p.a.win);
        float* cur = buf;           // after a transform: its result; the first pass of a transform writes `oth`
        float* oth = buf + 2 * P;
        const Lanes me{lane, lane + 1};
        frame_transform<BLUE>(me, M, P, p.npass, p.packed, tw, p.chirp, p.bhat, src, cur, oth, WaveBarrier{});
        untangle_lanes(me, M, cur, twn, oth, WaveBarrier{});
        mel_db_store(lane, p.a, oth, g, f);
    }
}

template <int LOG2M, typename Clips>
int launch_any(at_ctx* ctx, const AnyParams<Clips>& p, hipStream_t stream) {
    auto kernel = logmel_any_kernel<LOG2M, Clips>;
    constexpr int M = 1 << LOG2M, N = 2 * M;
    const size_t lds = ((size_t)6 * M + (size_t)(WG / 64) * (N + M + 4)) * sizeof(float);
    {
        const int rc = at_raise_lds(ctx, reinterpret_cast<const void*>(kernel), lds);
        if (rc) return rc;
    }
    // persistent: as many workgroups as fit the LDS of the chip (at most eight per CU), each wave walking frames
    long per_cu = (long)(160 * 1024 / lds);
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    long grid = per_cu * ctx->n_cus;
    const long need = (p.n_frames + WG / 64 - 1) / (WG / 64);
    if (grid > need) grid = need;
    AT_LAUNCH(kernel, dim3((unsigned)grid), dim3(WG), lds, stream, p);
    return AT_OK;
}

template <bool BLUE, typename Clips>
int launch_mixed(at_ctx* ctx, const MixedParams<Clips>& p, hipStream_t stream) {
    const size_t M = p.a.n_fft / 2, P = p.P;
    // as many waves per workgroup (at most four) as leave it inside a CU's 160 KiB of LDS
    const size_t tabs = (2 * P + 2 * M) * sizeof(float), per_wave = 4 * P * sizeof(float);
    int nw = WG / 64;
    while (nw > 1 && tabs + nw * per_wave > 160 * 1024) nw--;
    const size_t lds = tabs + nw * per_wave;
    if (lds > 160 * 1024) return at_fail(AT_E_INVALID, "at_logmel_f32: n_fft=%d needs %zu bytes of LDS", p.a.n_fft, lds);
    auto kernel = logmel_mixed_kernel<BLUE, Clips>;
    {
        const int rc = at_raise_lds(ctx, reinterpret_cast<const void*>(kernel), lds);
        if (rc) return rc;
    }
    long per_cu = (long)(160 * 1024 / lds);   // persistent, as the power-of-two kernel
    if (per_cu > 8) per_cu = 8;
    long grid = per_cu * ctx->n_cus;
    const long need = (p.a.n_frames + nw - 1) / nw;
    if (grid > need) grid = need;
    AT_LAUNCH(kernel, dim3((unsigned)grid), dim3(64 * nw), lds, stream, p);
    return AT_OK;
}

}  // namespace

// Tables for (sample_rate, n_fft, n_mels, filterbank values, form): window | W_M | W_N | form 2: W_P, chirp, filter
// transform | start, len, off | band weights.  Form 0 = a power of two (logmel_any_kernel), else lmx::Plan::form.
template <typename Clips>
int at_logmel_any(at_ctx* ctx, const Clips& clips, int64_t n_frames, int sample_rate, int n_fft, int hop, int n_mels,
                  const float* fb_user_dev, float* out, int frame_major, hipStream_t stream) {
    const int N = n_fft, M = N / 2, NBIN = M + 1;
    int log2m = 0;
    while ((1 << log2m) < M) log2m++;
    const bool pow2 = (N & (N - 1)) == 0;
    const Plan plan = make_plan(N, ctx->dbg.logmel_fallback != 0);
    const int form = pow2 ? 0 : plan.form;
    const int P = plan.P;
    const size_t head0 = (size_t)N + 2 * (size_t)M + 2 * (size_t)M;   // floats: window, W_M (M complex), W_N (M complex)
    const size_t head = head0 + (form == FORM_BLUESTEIN ? 2 * (size_t)P + 2 * (size_t)M + 2 * (size_t)P : 0);
    const lmt::BlobLayout lay = lmt::blob_layout(head, n_mels);
    const at_logmel_tables key{sample_rate, n_fft, n_mels, /* hop */ 0, form};
    const at_logmel_builder build = [&](const float* fb, std::vector<float>& blob, at_logmel_tables*) {
        blob.assign(head, 0.0f);
        lmt::hann_periodic(N, blob.data());
        twiddle_table(M, blob.data() + N);              // the builders the host harness checks (logmel_mixed_core.h)
        untangle_table(N, blob.data() + N + 2 * M);
        if (form == FORM_BLUESTEIN) {
            twiddle_table(P, blob.data() + head0);
            bluestein_tables(M, P, blob.data() + head0 + 2 * P, blob.data() + head0 + 2 * P + 2 * M);
        }
        lmt::pack_bands(blob, head, fb, NBIN, n_mels, 1);
    };
    const float* f = nullptr;
    int rc = at_logmel_resident(ctx, WS_LOGMEL_ANY, &ctx->lm_any, key, (lay.wts + (size_t)NBIN * n_mels) * 4, fb_user_dev,
                                stream, build, &f);
    if (rc) return rc;
    AnyParams<Clips> p;
    p.clips = clips;
    p.n_fft = N; p.log2m = log2m; p.hop = hop; p.n_mels = n_mels;
    p.n_frames = n_frames;
    p.win = f; p.twm = f + N; p.twn = f + N + 2 * M;
    p.fb_start = reinterpret_cast<const int*>(f + lay.ints);
    p.fb_len = p.fb_start + n_mels; p.fb_off = p.fb_start + 2 * n_mels;
    p.fb_wts = f + lay.wts;
    p.out = out; p.frame_major = frame_major;
    if (form != 0) {
        MixedParams<Clips> mp;
        mp.a = p;
        mp.P = P; mp.npass = plan.npass; mp.packed = plan.packed;
        mp.twp = form == FORM_BLUESTEIN ? f + head0 : p.twm;
        mp.chirp = f + head0 + 2 * P;
        mp.bhat = f + head0 + 2 * P + 2 * M;
        return form == FORM_BLUESTEIN ? launch_mixed<true>(ctx, mp, stream) : launch_mixed<false>(ctx, mp, stream);
    }
    switch (log2m) {
        case 5: return launch_any<5>(ctx, p, stream);
        case 6: return launch_any<6>(ctx, p, stream);
        case 7: return launch_any<7>(ctx, p, stream);
        case 8: return launch_any<8>(ctx, p, stream);
        case 9: return launch_any<9>(ctx, p, stream);
        case 10: return launch_any<10>(ctx, p, stream);
        case 11: return launch_any<11>(ctx, p, stream);
    }
    return at_fail(AT_E_INVALID, "at_logmel_f32: n_fft=%d not supported", n_fft);
}
template int at_logmel_any(at_ctx*, const lmc::UniformClips&, int64_t, int, int, int, int, const float*, float*, int, hipStream_t);
template int at_logmel_any(at_ctx*, const lmc::PlanClips&, int64_t, int, int, int, int, const float*, float*, int, hipStream_t);
