// mfcc.hip -- MFCC and delta features of log-mel rows: at_mfcc_f32, at_deltas_f32, at_dct_matrix_host.
//
// Contract (include/audio_tokens_amd.h repeats it).  Input: log-mel rows x[g][n], frame-major [n_frames][n_mels] fp32,
// and a device prefix first_frame[n_clips + 1] (int64, exclusive, last entry = n_frames); clip i owns the frames
// [first_frame[i], first_frame[i + 1]), empty clips allowed.
//   top_db       floor_i = (max over every value of clip i) - top_db, one fp32 subtraction; v < floor_i ? floor_i : v;
//                a clip that holds a NaN becomes NaN throughout.  The maximum is per clip, always.
//   table        dct[n][k], [n_mels][n_mfcc]: cos(pi / n_mels * (n + 0.5) * k) in double; ortho: column 0 scaled by
//                1/sqrt(2), then everything by sqrt(2 / n_mels); otherwise everything by 2; rounded to fp32 once.
//   coefficients c[g][k] = acc after acc = fmaf(x[g][n], dct[n][k], acc) for n = 0 .. n_mels - 1 ascending, from +0.
//   deltas       N = (win_length - 1) / 2; acc = +0; for j = 1 .. N ascending
//                acc = fmaf((float)j, c[clamp(t + j)] - c[clamp(t - j)], acc), clamp to the frame's own clip;
//                delta[t] = acc / denom, one IEEE division, denom = (float)(N (N + 1) (2N + 1) / 3).  The second order
//                is the same operator applied to the first.
//   output       D = n_mfcc * (1 + orders), feature o * n_mfcc + k; frame-major [n_frames][D], or feature-major: clip
//                i a contiguous [D][T_i] block at D * first_frame[i].
//
// Kernel.  One launch does the clamp, the DCT, both delta orders and the store.  A workgroup owns TB consecutive global
// frames (64; fewer only where the rows are too wide for that) and a halo of H = orders * N frames on each side.  A
// clamped neighbour always lies between a frame and its unclamped neighbour, so a tile needs nothing outside its
// halo and tiles need not be aligned to clips: every frame of the region finds its clip by binary search over the
// prefix, as lmc::find_clip does, and keeps the clip's bounds relative to the region.  The rows of tile and halo and the
// table are staged in LDS; thread (group of eight frames, pair of coefficients) runs sixteen chains at once from 16-byte
// reads of the rows and two reads of the table per step; coefficients, first and second order stay in LDS (odd row
// stride: both the k-fast reads of the deltas and the frame-fast reads of the feature-major store are conflict-free)
// until one store pass.
// Plain vector-ALU code, no MFMA: the call moves 4 * (n_mels + D) bytes per frame for 2 * n_mels * n_mfcc flops, far
// below what the vector ALU sustains, and the chain order is the contract either way.
// A table that does not fit beside the tile (more than MFCC_LDS_SMALL bytes in all) is read through L2 instead; rows
// wider still shrink TB and split the coefficients over blockIdx.y.  With the DCT stage compiled out (MODE 2) the
// same kernel is at_deltas_f32.
#include <cmath>

#include "at_internal.h"

namespace {

constexpr int WG = 256;
constexpr int FR = 8, KC = 2;                   // frames and coefficients per thread of the DCT stage
constexpr size_t MFCC_LDS_SMALL = 80 * 1024;    // table in LDS while two workgroups still fit on a CU
constexpr size_t MFCC_LDS_MAX = 156 * 1024;

// Ordered key of a float for an unsigned maximum: NaN above everything, 0 below everything (never a value's key).
__device__ __forceinline__ unsigned max_key(float v) {
    const unsigned b = __float_as_uint(v);
    if (v != v) return 0xFFFFFFFFu;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
    if (k == 0xFFFFFFFFu) return __builtin_nanf("");
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// the last clip whose prefix is <= g (a clip without frames is never found: lmc::find_clip)
__device__ __forceinline__ long find_clip(const long* __restrict__ first_frame, long n_clips, long g) {
    long lo = 0, hi = n_clips;
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (first_frame[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// keys[clip] = max over the clip's values (keys zeroed before).  A wave walks 16 consecutive frames, lanes over the
// mel index, and hands in one maximum per clip it met.
__global__ __launch_bounds__(WG) void mfcc_clip_max_kernel(const float* __restrict__ x, const long* __restrict__ first_frame,
                                                           long n_clips, long n_frames, int n_mels,
                                                           unsigned* __restrict__ keys) {
    const int lane = threadIdx.x & 63;
    long g = ((long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6)) * 16;
    const long ge = g + 16 < n_frames ? g + 16 : n_frames;
    while (g < ge) {
        const long clip = find_clip(first_frame, n_clips, g);
        long ce = first_frame[clip + 1];
        if (ce > ge) ce = ge;
        if (ce <= g) ce = g + 1;   // (a prefix that is not one: still terminates)
        unsigned m = 0;
        for (long f = g; f < ce; f++)
            for (int n = lane; n < n_mels; n += 64) {
                const unsigned k = max_key(x[f * n_mels + n]);
                m = k > m ? k : m;
            }
        for (int s = 32; s; s >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)m, s);
            m = o > m ? o : m;
        }
        if (lane == 0) atomicMax(&keys[clip], m);
        g = ce;
    }
}

struct MfccArgs {
    const float* x;            // [n_frames][n_in]
    const long* first_frame;   // [n_clips + 1]
    long n_clips, n_frames;
    const float* dct;          // [n_in][F] (MODE 0, 1)
    const unsigned* keys;      // per-clip maxima, or null: no top_db
    float* out;
    float top_db, denom;
    int n_in, F;               // floats per input row; coefficients per order
    int orders, o_lo, N;       // delta orders computed; first order that is stored; half window
    int feature_major, vec_in, vec_out;
    int TB, FC;                // frames per workgroup; coefficients per blockIdx.y
    int H, Nh, R;              // halo of the coefficients, of the first order; TB + 2H
    int xstride, Fs;           // LDS row strides: staged rows (multiple of 4), coefficient rows (odd)
    int off_a, off_tab, off_c; // LDS offsets in floats behind the per-frame records
};

// LDS: long cs[R], ce[R] (the clip's frames, global); int lo[R], hi[R] (the same, relative to the region and cut to
// it; lo == hi: no such frame); float fl[R] (top_db floor); A: the staged rows, later first order [(TB + 2 Nh)][Fs] and
// second order [TB][Fs]; the table [n_in][F] (MODE 0); c: coefficients [R][Fs].
// (LDS holds a compute unit to three workgroups or fewer, so the compiler may spend registers on loads in flight)
template <int MODE>
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(1, 4))) void mfcc_kernel(const MfccArgs a) {
    extern __shared__ float4 lds4[];
    long* cs = reinterpret_cast<long*>(lds4);
    long* ce = cs + a.R;
    int* lo = reinterpret_cast<int*>(ce + a.R);
    int* hi = lo + a.R;
    float* fl = reinterpret_cast<float*>(hi + a.R);
    float* lds = reinterpret_cast<float*>(lds4);
    float* A = lds + a.off_a;
    float* tab = lds + a.off_tab;
    float* c = lds + a.off_c;
    const int tid = threadIdx.x;
    const int R = a.R, F = a.F, Fs = a.Fs, H = a.H, N = a.N, Nh = a.Nh, TB = a.TB, n_in = a.n_in;
    const long g0 = (long)blockIdx.x * TB, rbase = g0 - H;
    const int k0 = blockIdx.y * a.FC;
    const int Fc = F - k0 < a.FC ? F - k0 : a.FC;

    for (int r = tid; r < R; r += WG) {
        const long g = rbase + r;
        long s = 0, e = 0;
        int l = 0, h = 0;
        float f = 0.0f;
        if (g >= 0 && g < a.n_frames) {
            const long clip = find_clip(a.first_frame, a.n_clips, g);
            s = a.first_frame[clip];
            e = a.first_frame[clip + 1];
            s = s < 0 ? 0 : (s > g ? g : s);                       // (whatever the prefix holds, the frame lies in
            e = e <= g ? g + 1 : (e > a.n_frames ? a.n_frames : e);   // its clip and the clip in the output)
            l = s - rbase < 0 ? 0 : (int)(s - rbase);
            h = e - rbase > R ? R : (int)(e - rbase);
            if (a.keys) f = key_value(a.keys[clip]) - a.top_db;
        }
        cs[r] = s, ce[r] = e, lo[r] = l, hi[r] = h, fl[r] = f;
    }
    __syncthreads();

    if (MODE == 2) {   // the rows are the coefficients
        for (int i = tid; i < R * Fc; i += WG) {
            const int r = i / Fc, kk = i - r * Fc;
            c[r * Fs + kk] = lo[r] < hi[r] ? a.x[(rbase + r) * n_in + k0 + kk] : 0.0f;
        }
    } else {
        const bool clampv = a.keys != nullptr;
        // (batches: the loads of a batch are all in flight before the first LDS store, which the compiler would
        // otherwise put between them)
        auto clamp = [&](float v, float f) { return f != f ? f : (v < f ? f : v); };
        if (a.vec_in) {
            const int nq = n_in >> 2, total = R * nq;
            for (int i0 = tid; i0 < total; i0 += 4 * WG) {
                float4 v[4];
                int dst[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int i = i0 + u * WG < total ? i0 + u * WG : total - 1;
                    const int r = i / nq, q = i - r * nq;
                    dst[u] = r * a.xstride + 4 * q;
                    v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (lo[r] < hi[r]) {
                        v[u] = *reinterpret_cast<const float4*>(a.x + (rbase + r) * n_in + 4 * q);
                        if (clampv) {
                            const float f = fl[r];
                            v[u] = make_float4(clamp(v[u].x, f), clamp(v[u].y, f), clamp(v[u].z, f), clamp(v[u].w, f));
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (i0 + u * WG < total) *reinterpret_cast<float4*>(A + dst[u]) = v[u];
            }
        } else {
            const int total = R * n_in;
            for (int i0 = tid; i0 < total; i0 += 8 * WG) {
                float v[8];
                int dst[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int i = i0 + u * WG < total ? i0 + u * WG : total - 1;
                    const int r = i / n_in, n = i - r * n_in;
                    dst[u] = r * a.xstride + n;
                    v[u] = 0.0f;
                    if (lo[r] < hi[r]) {
                        v[u] = a.x[(rbase + r) * n_in + n];
                        if (clampv) v[u] = clamp(v[u], fl[r]);
                    }
                }
#pragma unroll
                for (int u = 0; u < 8; u++)
                    if (i0 + u * WG < total) A[dst[u]] = v[u];
            }
        }
        if (MODE == 0) {
            const int total = n_in * F;
            for (int i0 = tid; i0 < total; i0 += 8 * WG) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = a.dct[i0 + u * WG < total ? i0 + u * WG : total - 1];
#pragma unroll
                for (int u = 0; u < 8; u++)
                    if (i0 + u * WG < total) tab[i0 + u * WG] = v[u];
            }
        }
        __syncthreads();

        // thread (group of FR frames, pair of coefficients): FR * KC chains at once, each ascending in n
        const float* __restrict__ t = MODE == 0 ? tab : a.dct;
        const int nkp = (Fc + KC - 1) / KC;
        const int items = ((R + FR - 1) / FR) * nkp;
        for (int it = tid; it < items; it += WG) {
            const int fg = it / nkp, kk = (it - fg * nkp) * KC;
            const int r0 = fg * FR;
            const bool two = kk + 1 < Fc;
            const float* tk0 = t + k0 + kk;
            const float* tk1 = tk0 + (two ? 1 : 0);
            const float* xr[FR];
#pragma unroll
            for (int i = 0; i < FR; i++) xr[i] = A + (r0 + i < R ? r0 + i : R - 1) * a.xstride;
            float acc[FR][KC];
#pragma unroll
            for (int i = 0; i < FR; i++) acc[i][0] = acc[i][1] = 0.0f;
            int n = 0;
            for (; n + 4 <= n_in; n += 4) {
                float ta[4], tb[4];
#pragma unroll
                for (int u = 0; u < 4; u++) ta[u] = tk0[(size_t)(n + u) * F], tb[u] = tk1[(size_t)(n + u) * F];
                float4 v[FR];   // (all reads in flight before the first use: the waves are few, the chains long)
#pragma unroll
                for (int i = 0; i < FR; i++) v[i] = *reinterpret_cast<const float4*>(xr[i] + n);
#pragma unroll
                for (int i = 0; i < FR; i++) {
                    acc[i][0] = __builtin_fmaf(v[i].x, ta[0], acc[i][0]), acc[i][1] = __builtin_fmaf(v[i].x, tb[0], acc[i][1]);
                    acc[i][0] = __builtin_fmaf(v[i].y, ta[1], acc[i][0]), acc[i][1] = __builtin_fmaf(v[i].y, tb[1], acc[i][1]);
                    acc[i][0] = __builtin_fmaf(v[i].z, ta[2], acc[i][0]), acc[i][1] = __builtin_fmaf(v[i].z, tb[2], acc[i][1]);
                    acc[i][0] = __builtin_fmaf(v[i].w, ta[3], acc[i][0]), acc[i][1] = __builtin_fmaf(v[i].w, tb[3], acc[i][1]);
                }
            }
            for (; n < n_in; n++) {
                const float t0 = tk0[(size_t)n * F], t1 = tk1[(size_t)n * F];
#pragma unroll
                for (int i = 0; i < FR; i++) {
                    const float v = xr[i][n];
                    acc[i][0] = __builtin_fmaf(v, t0, acc[i][0]), acc[i][1] = __builtin_fmaf(v, t1, acc[i][1]);
                }
            }
#pragma unroll
            for (int i = 0; i < FR; i++)
                if (r0 + i < R) {
                    c[(r0 + i) * Fs + kk] = acc[i][0];
                    if (two) c[(r0 + i) * Fs + kk + 1] = acc[i][1];
                }
        }
    }
    __syncthreads();   // (the staged rows are dead from here: A becomes d1, d2)

    float* d1 = A;                           // rows H - Nh .. H + TB + Nh of the region
    float* d2 = A + (TB + 2 * Nh) * Fs;      // rows H .. H + TB
    if (a.orders >= 1) {
        const int rows = TB + 2 * Nh;
        for (int i = tid; i < rows * Fc; i += WG) {
            const int q = i / Fc, kk = i - q * Fc;
            const int r = q + H - Nh;
            const int l = lo[r], h = hi[r];
            float v = 0.0f;
            if (l < h) {
                float acc = 0.0f;
                for (int j = 1; j <= N; j++) {
                    const int ip = r + j < h ? r + j : h - 1, im = r - j > l ? r - j : l;
                    const float diff = c[ip * Fs + kk] - c[im * Fs + kk];
                    acc = __builtin_fmaf((float)j, diff, acc);
                }
                v = acc / a.denom;
            }
            d1[q * Fs + kk] = v;
        }
        __syncthreads();
    }
    if (a.orders >= 2) {
        const int off = H - Nh;              // d1's row q is row q + off of the region
        for (int i = tid; i < TB * Fc; i += WG) {
            const int tt = i / Fc, kk = i - tt * Fc;
            const int q = tt + Nh;
            const int l = lo[H + tt] - off, h = hi[H + tt] - off;
            float v = 0.0f;
            if (l < h) {
                float acc = 0.0f;
                for (int j = 1; j <= N; j++) {
                    const int ip = q + j < h ? q + j : h - 1;
                    int im = q - j > l ? q - j : l;
                    im = im < 0 ? 0 : im;    // (never taken for a frame that is stored: q - j >= 0)
                    const float diff = d1[ip * Fs + kk] - d1[im * Fs + kk];
                    acc = __builtin_fmaf((float)j, diff, acc);
                }
                v = acc / a.denom;
            }
            d2[tt * Fs + kk] = v;
        }
        __syncthreads();
    }

    // the store: order o of frame tt is c[H + tt], d1[Nh + tt], d2[tt]
    const long left = a.n_frames - g0;
    const int tv = left < TB ? (int)left : TB;
    const int no = a.orders + 1 - a.o_lo;
    const int D = no * F, Dc = no * Fc;
    const float *s0 = c + H * Fs, *s1 = d1 + Nh * Fs;
    auto src = [&](int o) { return o == 0 ? s0 : (o == 1 ? s1 : d2); };
    if (a.feature_major) {
        for (int i = tid; i < Dc * TB; i += WG) {
            const int fe = i / TB, tt = i - fe * TB;
            if (tt >= tv) continue;
            const int oo = fe / Fc, kk = fe - oo * Fc;
            const long s = cs[H + tt], T = ce[H + tt] - s;
            a.out[D * s + (long)(oo * F + k0 + kk) * T + (g0 + tt - s)] = src(oo + a.o_lo)[tt * Fs + kk];
        }
    } else if (a.vec_out) {   // one block in y: the tile's floats are one contiguous run
        float4* o4 = reinterpret_cast<float4*>(a.out + g0 * D);
        const int D4 = D >> 2;
        for (int i = tid; i < tv * D4; i += WG) {
            const int tt = i / D4, fe = (i - tt * D4) * 4;
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int f = fe + u;
                const int oo = (f >= F) + (f >= 2 * F);
                v[u] = src(oo + a.o_lo)[tt * Fs + f - oo * F];
            }
            o4[i] = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (int i = tid; i < tv * Dc; i += WG) {
            const int tt = i / Dc, fe = i - tt * Dc;
            const int oo = fe / Fc, kk = fe - oo * Fc;
            a.out[(g0 + tt) * D + oo * F + k0 + kk] = src(oo + a.o_lo)[tt * Fs + kk];
        }
    }
}

size_t plan_bytes(MfccArgs* a, int mode, int TB, int FC) {
    a->TB = TB, a->FC = FC;
    a->R = TB + 2 * a->H;
    a->Fs = FC | 1;
    a->xstride = mode == 2 ? 0 : ((a->n_in + 3) & ~3) + 4;
    size_t head = (size_t)a->R * (2 * sizeof(long) + 2 * sizeof(int) + sizeof(float));
    head = (head + 15) & ~(size_t)15;
    const size_t d12 = (size_t)((a->orders >= 1 ? TB + 2 * a->Nh : 0) + (a->orders >= 2 ? TB : 0)) * a->Fs;
    const size_t rows = (size_t)a->R * a->xstride;
    size_t fa = rows > d12 ? rows : d12;
    fa = (fa + 3) & ~(size_t)3;
    const size_t ft = mode == 0 ? (((size_t)a->n_in * a->F + 3) & ~(size_t)3) : 0;
    a->off_a = (int)(head / sizeof(float));
    a->off_tab = a->off_a + (int)fa;
    a->off_c = a->off_tab + (int)ft;
    return head + sizeof(float) * (fa + ft + (size_t)a->R * a->Fs);
}

// Picks the form (*mode: 0 table in LDS, 1 table through L2; 2 stays 2), TB and FC; false: the halo does not fit.
bool plan(MfccArgs* a, int* mode, size_t* bytes) {
    if (*mode != 2) {
        *mode = 0;
        *bytes = plan_bytes(a, 0, 64, a->F);
        if (*bytes <= MFCC_LDS_SMALL) return true;
        *mode = 1;
    }
    for (int TB = 64; TB >= 8; TB >>= 1)
        for (int FC = a->F;; FC = (FC + 1) / 2) {
            *bytes = plan_bytes(a, *mode, TB, FC);
            if (*bytes <= MFCC_LDS_MAX && (a->F + FC - 1) / FC <= 65535) return true;
            if (FC == 1) break;
        }
    return false;
}

int launch(at_ctx* ctx, MfccArgs& a, int mode, const char* who, hipStream_t stream) {
    size_t bytes = 0;
    AT_REQUIRE(plan(&a, &mode, &bytes), "%s: win_length=%d needs more LDS than a compute unit has beside rows of %d floats",
               who, 2 * a.N + 1, a.n_in);
    const int no = a.orders + 1 - a.o_lo;
    const unsigned ny = (unsigned)((a.F + a.FC - 1) / a.FC);
    a.vec_in = mode != 2 && a.n_in % 4 == 0 && at_aligned16(a.x);
    a.vec_out = !a.feature_major && ny == 1 && (no * a.F) % 4 == 0 && at_aligned16(a.out);
    const int64_t nb = (a.n_frames + a.TB - 1) / a.TB;
    AT_REQUIRE(nb <= 0x7FFFFFFF, "%s: n_frames=%lld too large", who, (long long)a.n_frames);
    const dim3 grid((unsigned)nb, ny);
    if (mode == 0) {
        AT_RAISE_LDS(ctx, mfcc_kernel<0>, bytes);
        AT_LAUNCH(mfcc_kernel<0>, grid, dim3(WG), bytes, stream, a);
    } else if (mode == 1) {
        AT_RAISE_LDS(ctx, mfcc_kernel<1>, bytes);
        AT_LAUNCH(mfcc_kernel<1>, grid, dim3(WG), bytes, stream, a);
    } else {
        AT_RAISE_LDS(ctx, mfcc_kernel<2>, bytes);
        AT_LAUNCH(mfcc_kernel<2>, grid, dim3(WG), bytes, stream, a);
    }
    return AT_OK;
}

float delta_denom(int N) { return (float)((int64_t)N * (N + 1) * (2 * N + 1) / 3); }

}  // namespace

extern "C" int at_dct_matrix_host(int n_mfcc, int n_mels, int ortho, float* dct_host) {
    AT_REQUIRE(dct_host, "at_dct_matrix_host: null pointer");
    AT_REQUIRE(n_mels >= 1 && n_mfcc >= 1 && n_mfcc <= n_mels, "at_dct_matrix_host: bad sizes n_mfcc=%d n_mels=%d", n_mfcc,
               n_mels);
    const double pi = 3.14159265358979323846;
    const double scale = ortho ? std::sqrt(2.0 / n_mels) : 2.0;
    for (int n = 0; n < n_mels; n++)
        for (int k = 0; k < n_mfcc; k++) {
            double v = std::cos(pi / n_mels * (n + 0.5) * k);
            if (ortho && k == 0) v *= 1.0 / std::sqrt(2.0);
            dct_host[(size_t)n * n_mfcc + k] = (float)(v * scale);
        }
    return AT_OK;
}

extern "C" int at_mfcc_f32(at_ctx* ctx, const float* logmel, const int64_t* first_frame, int64_t n_clips, int64_t n_frames,
                           int n_mels, int n_mfcc, const float* dct_or_null, int orders, int win_length, int use_top_db,
                           float top_db, float* out, int layout, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_mfcc_f32: ctx is null");
    AT_REQUIRE(n_clips >= 0 && n_frames >= 0 && n_clips <= 0x7FFFFFFF, "at_mfcc_f32: bad sizes n_clips=%lld n_frames=%lld",
               (long long)n_clips, (long long)n_frames);
    AT_REQUIRE(n_mels >= 1 && n_mels <= 1024, "at_mfcc_f32: n_mels=%d out of range", n_mels);
    AT_REQUIRE(n_mfcc >= 1 && n_mfcc <= n_mels, "at_mfcc_f32: n_mfcc=%d outside [1, n_mels=%d]", n_mfcc, n_mels);
    AT_REQUIRE(orders >= 0 && orders <= 2, "at_mfcc_f32: orders=%d outside 0..2", orders);
    AT_REQUIRE(win_length >= 3 && win_length % 2 == 1, "at_mfcc_f32: win_length=%d must be odd and >= 3", win_length);
    AT_REQUIRE(!use_top_db || top_db >= 0.0f, "at_mfcc_f32: top_db=%g must not be negative", (double)top_db);
    AT_REQUIRE(layout == AT_LAYOUT_MEL_MAJOR || layout == AT_LAYOUT_FRAME_MAJOR, "at_mfcc_f32: unknown layout %d", layout);
    if (n_frames == 0 || n_clips == 0) return AT_OK;
    AT_REQUIRE(logmel && first_frame && out, "at_mfcc_f32: null pointer");
    AT_REQUIRE(n_frames <= ((int64_t)1 << 38) / (3 * n_mels), "at_mfcc_f32: n_frames=%lld too large", (long long)n_frames);
    AT_HIP(hipSetDevice(ctx->device));

    MfccArgs a{};
    a.x = logmel, a.first_frame = reinterpret_cast<const long*>(first_frame), a.n_clips = n_clips, a.n_frames = n_frames;
    a.dct = dct_or_null, a.out = out, a.top_db = top_db;
    a.n_in = n_mels, a.F = n_mfcc, a.orders = orders, a.o_lo = 0, a.N = orders ? (win_length - 1) / 2 : 0;
    a.denom = orders ? delta_denom(a.N) : 1.0f;
    a.H = orders * a.N, a.Nh = orders == 2 ? a.N : 0;
    a.feature_major = layout == AT_LAYOUT_MEL_MAJOR;

    const bool guarded = use_top_db || !dct_or_null;
    if (guarded) {
        const int rc = at_guard_enter(&ctx->guard[AT_GUARD_MFCC], stream);
        if (rc) return rc;
    }
    if (!dct_or_null) {
        const size_t bytes = sizeof(float) * (size_t)n_mels * n_mfcc;
        float* tab = static_cast<float*>(at_ws(ctx, WS_MFCC_DCT, bytes, stream));
        if (!tab) return AT_E_NOMEM;
        if (ctx->mfcc_dct_nmfcc != n_mfcc || ctx->mfcc_dct_nmels != n_mels) {
            std::vector<float> host((size_t)n_mels * n_mfcc);
            at_dct_matrix_host(n_mfcc, n_mels, 1, host.data());
            ctx->mfcc_dct_nmfcc = ctx->mfcc_dct_nmels = 0;
            AT_HIP(hipMemcpyAsync(tab, host.data(), bytes, hipMemcpyHostToDevice, stream));
            AT_HIP(hipStreamSynchronize(stream));   // (the source is a temporary; once per table)
            ctx->mfcc_dct_nmfcc = n_mfcc, ctx->mfcc_dct_nmels = n_mels;
        }
        a.dct = tab;
    }
    if (use_top_db) {
        unsigned* keys = static_cast<unsigned*>(at_ws(ctx, WS_MFCC_MAX, sizeof(unsigned) * (size_t)n_clips, stream));
        if (!keys) return AT_E_NOMEM;
        AT_HIP(hipMemsetAsync(keys, 0, sizeof(unsigned) * (size_t)n_clips, stream));
        const int64_t per_block = 16 * (WG / 64);
        AT_LAUNCH(mfcc_clip_max_kernel, dim3((unsigned)((n_frames + per_block - 1) / per_block)), dim3(WG), 0, stream, logmel,
                  a.first_frame, (long)n_clips, (long)n_frames, n_mels, keys);
        a.keys = keys;
    }
    const int rc = launch(ctx, a, 0, "at_mfcc_f32", stream);
    if (rc) return rc;
    return guarded ? at_guard_leave(&ctx->guard[AT_GUARD_MFCC], stream) : AT_OK;
}

extern "C" int at_deltas_f32(at_ctx* ctx, const float* rows, const int64_t* first_frame, int64_t n_clips, int64_t n_frames,
                             int F, int win_length, float* out, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_deltas_f32: ctx is null");
    AT_REQUIRE(n_clips >= 0 && n_frames >= 0 && n_clips <= 0x7FFFFFFF && F >= 1,
               "at_deltas_f32: bad sizes n_clips=%lld n_frames=%lld F=%d", (long long)n_clips, (long long)n_frames, F);
    AT_REQUIRE(win_length >= 3 && win_length % 2 == 1, "at_deltas_f32: win_length=%d must be odd and >= 3", win_length);
    if (n_frames == 0 || n_clips == 0) return AT_OK;
    AT_REQUIRE(rows && first_frame && out, "at_deltas_f32: null pointer");
    AT_REQUIRE(n_frames <= ((int64_t)1 << 38) / F, "at_deltas_f32: n_frames=%lld too large", (long long)n_frames);
    AT_HIP(hipSetDevice(ctx->device));
    MfccArgs a{};
    a.x = rows, a.first_frame = reinterpret_cast<const long*>(first_frame), a.n_clips = n_clips, a.n_frames = n_frames;
    a.out = out, a.n_in = F, a.F = F, a.orders = 1, a.o_lo = 1, a.N = (win_length - 1) / 2;
    a.denom = delta_denom(a.N);
    a.H = a.N, a.Nh = 0;
    return launch(ctx, a, 2, "at_deltas_f32", stream);
}
