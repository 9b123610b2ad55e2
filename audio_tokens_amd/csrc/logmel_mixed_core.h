// logmel_mixed_core.h -- plan and per-lane arithmetic of the general log-mel kernels (logmel_any.hip).
//
// The real n_fft-point transform of a frame is the M = n_fft/2-point complex FFT of z[m] = x[2m] + i x[2m+1] plus the
// even/odd untangling.  For the even n_fft that are not powers of two, M is any integer from 32 to 2048 and the
// complex transform takes one of two forms:
//   form 1 (mixed radix)  M = 2^a 3^b 5^c 7^d: Stockham passes of radix 8, 4, 2, 3, 5, 7 chosen at run time, out of
//                         place between two buffers (a pass reads one and writes the other, so nothing depends on how
//                         many butterflies a lane holds);
//   form 2 (Bluestein)    every other M: Z[k] = w[k] * sum_n (z[n] w[n]) conj(w[k-n]) with the chirp
//                         w[n] = exp(-i pi n^2 / M), the convolution done by two power-of-two transforms of
//                         P >= 2M - 1 points built from the same passes (radix 8, 4, 2).
// Everything is written from the point of view of ONE lane of the wavefront that owns the frame and touches memory only
// through the load / store functors it is given, so the same code runs in the HIP kernel (LDS, global memory) and,
// lane after lane, in tests/host_harness/logmel_mixed_host.cpp, which checks the index algebra of every size against
// numpy without a GPU.  Tables are computed in double on the host and rounded to fp32.
#pragma once

#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define AT_MX_HD __host__ __device__ __forceinline__
#else
#define AT_MX_HD inline
#endif

namespace lmx {

struct cx {
    float re, im;
};
AT_MX_HD cx cadd(cx a, cx b) { return {a.re + b.re, a.im + b.im}; }
AT_MX_HD cx csub(cx a, cx b) { return {a.re - b.re, a.im - b.im}; }
// fused multiply-adds are written out (the library is compiled with -ffp-contract=off)
AT_MX_HD cx cmul(cx a, cx w) {
    return {__builtin_fmaf(a.re, w.re, -(a.im * w.im)), __builtin_fmaf(a.re, w.im, a.im * w.re)};
}
AT_MX_HD cx cconj(cx a) { return {a.re, -a.im}; }

// forward DFTs in registers, natural order in and out
AT_MX_HD void dft2(cx (&v)[2]) {
    const cx a = v[0], b = v[1];
    v[0] = cadd(a, b);
    v[1] = csub(a, b);
}
AT_MX_HD void dft4(cx& a, cx& b, cx& c, cx& d) {
    const cx t0 = cadd(a, c), t1 = csub(a, c), t2 = cadd(b, d), t3 = csub(b, d);
    a = cadd(t0, t2);
    c = csub(t0, t2);
    b = {t1.re + t3.im, t1.im - t3.re};  // t1 - i*t3
    d = {t1.re - t3.im, t1.im + t3.re};  // t1 + i*t3
}
AT_MX_HD void dft4(cx (&v)[4]) { dft4(v[0], v[1], v[2], v[3]); }
AT_MX_HD void dft8(cx (&v)[8]) {
    constexpr float R2 = 0.70710678118654752f;
    dft4(v[0], v[2], v[4], v[6]);   // E[0..3] left at v[0], v[2], v[4], v[6]
    dft4(v[1], v[3], v[5], v[7]);   // O[0..3] left at v[1], v[3], v[5], v[7]
    const cx o0 = v[1];
    const cx o1 = {R2 * (v[3].re + v[3].im), R2 * (v[3].im - v[3].re)};      // * W8^1 = (1 - i)/sqrt 2
    const cx o2 = {v[5].im, -v[5].re};                                        // * W8^2 = -i
    const cx o3 = {R2 * (v[7].im - v[7].re), -R2 * (v[7].re + v[7].im)};     // * W8^3 = (-1 - i)/sqrt 2
    const cx e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
    v[0] = cadd(e0, o0); v[4] = csub(e0, o0);
    v[1] = cadd(e1, o1); v[5] = csub(e1, o1);
    v[2] = cadd(e2, o2); v[6] = csub(e2, o2);
    v[3] = cadd(e3, o3); v[7] = csub(e3, o3);
}

// cos / sin of 2 pi j / R for the odd radices (j = 0 .. R-1)
template <int R>
AT_MX_HD constexpr float odd_cos(int j) {
    if (R == 3) {
        constexpr float t[3] = {1.0f, -0.5f, -0.5f};
        return t[j];
    } else if (R == 5) {
        constexpr float t[5] = {1.0f, 0.30901699437494742f, -0.80901699437494742f, -0.80901699437494742f,
                                0.30901699437494742f};
        return t[j];
    } else {
        constexpr float t[7] = {1.0f, 0.62348980185873353f, -0.22252093395631440f, -0.90096886790241913f,
                                -0.90096886790241913f, -0.22252093395631440f, 0.62348980185873353f};
        return t[j];
    }
}
template <int R>
AT_MX_HD constexpr float odd_sin(int j) {
    if (R == 3) {
        constexpr float t[3] = {0.0f, 0.86602540378443865f, -0.86602540378443865f};
        return t[j];
    } else if (R == 5) {
        constexpr float t[5] = {0.0f, 0.95105651629515357f, 0.58778525229247313f, -0.58778525229247313f,
                                -0.95105651629515357f};
        return t[j];
    } else {
        constexpr float t[7] = {0.0f, 0.78183148246802981f, 0.97492791218182361f, 0.43388373911755812f,
                                -0.43388373911755812f, -0.97492791218182361f, -0.78183148246802981f};
        return t[j];
    }
}
// Odd prime radix: with t_n = x[n] + x[R-n], u_n = x[n] - x[R-n] (n = 1 .. (R-1)/2),
//   X[k], X[R-k] = (x[0] + sum_n cos(2 pi k n / R) t_n)  -/+  i (sum_n sin(2 pi k n / R) u_n).
template <int R>
AT_MX_HD void dft_odd(cx (&v)[R]) {
    constexpr int H = (R - 1) / 2;
    cx t[H], u[H];
#pragma unroll
    for (int n = 0; n < H; n++) {
        t[n] = cadd(v[n + 1], v[R - 1 - n]);
        u[n] = csub(v[n + 1], v[R - 1 - n]);
    }
    const cx a = v[0];
    cx s = a;
#pragma unroll
    for (int n = 0; n < H; n++) s = cadd(s, t[n]);
    v[0] = s;
#pragma unroll
    for (int k = 1; k <= H; k++) {
        cx m = a, q = {0.0f, 0.0f};
#pragma unroll
        for (int n = 1; n <= H; n++) {
            const float c = odd_cos<R>((k * n) % R), sn = odd_sin<R>((k * n) % R);
            m = {__builtin_fmaf(c, t[n - 1].re, m.re), __builtin_fmaf(c, t[n - 1].im, m.im)};
            q = {__builtin_fmaf(sn, u[n - 1].re, q.re), __builtin_fmaf(sn, u[n - 1].im, q.im)};
        }
        v[k] = {m.re + q.im, m.im - q.re};       // m - i q
        v[R - k] = {m.re - q.im, m.im + q.re};   // m + i q
    }
}
template <int R>
AT_MX_HD void dftR(cx (&v)[R]) {
    if constexpr (R == 8) dft8(v);
    else if constexpr (R == 4) dft4(v);
    else if constexpr (R == 2) dft2(v);
    else dft_odd<R>(v);
}

// ---- plan ----------------------------------------------------------------------------------------------------------
constexpr int MAX_PASSES = 11;
constexpr int FORM_MIXED = 1, FORM_BLUESTEIN = 2;

struct Plan {
    int M;                    // n_fft / 2: points of the complex transform
    int form;                 // FORM_MIXED / FORM_BLUESTEIN
    int P;                    // points of the Stockham passes: M (form 1) or the power of two >= 2M - 1 (form 2)
    int npass;
    int radix[MAX_PASSES];    // product = P
    uint64_t packed;          // radix[i] in bits 4i .. 4i+3 (a kernel argument that needs no indexed array)
};

// radix 8 while 8 divides what is left, then 4 or 2, then 3s, 5s and 7s; *left = what none of them divides
inline int factor_smooth(int n, int* radix, int* left) {
    int np = 0;
    const int order[6] = {8, 4, 2, 3, 5, 7};
    for (int r : order)
        while (n % r == 0 && np < MAX_PASSES) {
            radix[np++] = r;
            n /= r;
        }
    *left = n;
    return np;
}

// n_fft even, 64 .. 4096.  force_fallback: form 2 for the smooth sizes too.
inline Plan make_plan(int n_fft, bool force_fallback) {
    Plan pl{};
    pl.M = n_fft / 2;
    int left = 0;
    pl.npass = factor_smooth(pl.M, pl.radix, &left);
    if (left == 1 && !force_fallback) {
        pl.form = FORM_MIXED;
        pl.P = pl.M;
    } else {
        pl.form = FORM_BLUESTEIN;
        pl.P = 1;
        while (pl.P < 2 * pl.M - 1) pl.P *= 2;
        pl.npass = factor_smooth(pl.P, pl.radix, &left);
    }
    for (int i = pl.npass; i < MAX_PASSES; i++) pl.radix[i] = 0;
    pl.packed = 0;
    for (int i = 0; i < pl.npass; i++) pl.packed |= (uint64_t)pl.radix[i] << (4 * i);
    return pl;
}
AT_MX_HD int plan_radix(uint64_t packed, int i) { return (int)((packed >> (4 * i)) & 15u); }

// ---- one Stockham pass, one lane ------------------------------------------------------------------------------------
// Butterfly j (of NB = P/R) takes the inputs j + t*NB, multiplies input t by W_(NS*R)^(k*t) = W_P^(k*t*P/(NS*R)) with
// k = j mod NS (NS = product of the radices before this pass), and leaves the R outputs at (j - k)*R + k + t*NS.
// Natural order in, natural order out after the last pass.  j mod NS in fp32 ((j + 1/2) / NS is at least 1/(2 NS) away
// from an integer and j/NS <= 2048/NS: five decimal orders above the rounding error), then put right if it is off by one.
AT_MX_HD int mod_ns(int j, int NS, float inv_ns) {
    int k = j - (int)(((float)j + 0.5f) * inv_ns) * NS;
    if (k < 0) k += NS;
    if (k >= NS) k -= NS;
    return k;
}

template <int R, typename Load, typename Store>
AT_MX_HD void butterfly(int j, int NB, int NS, float inv_ns, int tstride, const float* tw, Load load, Store store) {
    cx v[R];
#pragma unroll
    for (int t = 0; t < R; t++) v[t] = load(j + t * NB);
    int k = 0;
    if (NS > 1) {
        k = mod_ns(j, NS, inv_ns);
        const int q1 = k * tstride;
#pragma unroll
        for (int t = 1; t < R; t++) v[t] = cmul(v[t], {tw[2 * (q1 * t)], tw[2 * (q1 * t) + 1]});
    }
    dftR<R>(v);
    const int j0 = (j - k) * R + k;
#pragma unroll
    for (int t = 0; t < R; t++) store(j0 + t * NS, v[t]);
}

// the butterflies lane, lane + 64, ... of one pass.  POW2: only the radices of a power-of-two plan are instantiated.
template <bool POW2, typename Load, typename Store>
AT_MX_HD void pass_lane(int lane, int P, int R, int NS, const float* tw, Load load, Store store) {
    const int NB = P / R, tstride = NB / NS;
    const float inv_ns = 1.0f / (float)NS;
    switch (R) {
        case 8: for (int j = lane; j < NB; j += 64) butterfly<8>(j, NB, NS, inv_ns, tstride, tw, load, store); break;
        case 4: for (int j = lane; j < NB; j += 64) butterfly<4>(j, NB, NS, inv_ns, tstride, tw, load, store); break;
        case 2: for (int j = lane; j < NB; j += 64) butterfly<2>(j, NB, NS, inv_ns, tstride, tw, load, store); break;
        default:
            if constexpr (!POW2) {
                if (R == 3) for (int j = lane; j < NB; j += 64) butterfly<3>(j, NB, NS, inv_ns, tstride, tw, load, store);
                else if (R == 5) for (int j = lane; j < NB; j += 64) butterfly<5>(j, NB, NS, inv_ns, tstride, tw, load, store);
                else for (int j = lane; j < NB; j += 64) butterfly<7>(j, NB, NS, inv_ns, tstride, tw, load, store);
            }
    }
}

struct LdsLoad {
    const float* z;
    AT_MX_HD cx operator()(int i) const { return {z[2 * i], z[2 * i + 1]}; }
};
struct LdsStore {
    float* z;
    AT_MX_HD void operator()(int i, cx v) const {
        z[2 * i] = v.re;
        z[2 * i + 1] = v.im;
    }
};

// Bluestein, second transform's input: conj(A[i] * Bhat[i]) -- the inverse transform is conj(FFT(conj(.))), its 1/P
// is folded into Bhat.
struct BlueProductLoad {
    const float* a;      // FFT_P of the chirped, zero-padded frame
    const float* bhat;   // FFT_P of the wrapped conj chirp, / P
    AT_MX_HD cx operator()(int i) const {
        return cconj(cmul({a[2 * i], a[2 * i + 1]}, {bhat[2 * i], bhat[2 * i + 1]}));
    }
};
// Bluestein, last step: Z[k] = w[k] * conj(c'[k])
AT_MX_HD cx blue_finish(cx cprime, cx wk) { return cmul(cconj(cprime), wk); }

// Bluestein, first transform's input: the frame times the chirp, zero-padded to P points
template <typename Src>
struct BlueChirpLoad {
    Src src;
    const float* chirp;
    int M;
    AT_MX_HD cx operator()(int m) const {
        if (m >= M) return cx{0.0f, 0.0f};
        return cmul(src(m), {chirp[2 * m], chirp[2 * m + 1]});
    }
};

// ---- a frame's sequence of passes ----------------------------------------------------------------------------------
// The lanes the caller stands for: its own lane of the wavefront in the kernel (begin = lane, end = lane + 1), all 64
// one after the other in the host harness.  `barrier` is called where every lane must have finished what was written
// before anybody reads it: the wave barrier in the kernel (a wavefront's LDS instructions execute in order; the barrier
// keeps the compiler from moving an access across it), nothing on the host.
struct Lanes {
    int begin, end;
};

// All passes of a plan.  The first reads through `first`, the others read `cur`; every pass writes `oth`, then the two
// change places: on return `cur` holds the transform in natural order and `oth` is free.
template <bool POW2, typename Load, typename Barrier>
AT_MX_HD void run_passes(Lanes ln, int P, int npass, uint64_t packed, const float* tw, Load first, float*& cur,
                         float*& oth, Barrier barrier) {
    int NS = 1;
    for (int i = 0; i < npass; i++) {
        const int R = plan_radix(packed, i);
        for (int lane = ln.begin; lane < ln.end; lane++) {
            if (i == 0) pass_lane<POW2>(lane, P, R, NS, tw, first, LdsStore{oth});
            else pass_lane<POW2>(lane, P, R, NS, tw, LdsLoad{cur}, LdsStore{oth});
        }
        barrier();
        float* s = cur; cur = oth; oth = s;
        NS *= R;
    }
}

// Z = the M-point transform of the frame `src` yields (complex point m = src(m)), left in `cur`; `cur` and `oth` are
// the wave's two buffers of P complex points.  BLUE = false: P = M, the passes themselves.  BLUE = true: the frame
// times the chirp through P-point passes, the product with `bhat` (read from `cur` by the first pass of the second
// transform, which writes `oth`) through the passes again, then Z[k] = w[k] conj(c'[k]) into the free buffer.
template <bool BLUE, typename Src, typename Barrier>
AT_MX_HD void frame_transform(Lanes ln, int M, int P, int npass, uint64_t packed, const float* tw, const float* chirp,
                              const float* bhat, Src src, float*& cur, float*& oth, Barrier barrier) {
    if constexpr (!BLUE) {
        run_passes<false>(ln, P, npass, packed, tw, src, cur, oth, barrier);
    } else {
        run_passes<true>(ln, P, npass, packed, tw, BlueChirpLoad<Src>{src, chirp, M}, cur, oth, barrier);
        run_passes<true>(ln, P, npass, packed, tw, BlueProductLoad{cur, bhat}, cur, oth, barrier);
        for (int lane = ln.begin; lane < ln.end; lane++)
            for (int k = lane; k < M; k += 64) {
                const cx v = blue_finish({cur[2 * k], cur[2 * k + 1]}, {chirp[2 * k], chirp[2 * k + 1]});
                oth[2 * k] = v.re;
                oth[2 * k + 1] = v.im;
            }
        barrier();
        float* s = cur; cur = oth; oth = s;
    }
}

// ---- even / odd untangling ------------------------------------------------------------------------------------------
// X[k] = Ev + W_N^k * Od, Ev = (Z[k] + conj Z[M-k]) / 2, Od = -i (Z[k] - conj Z[M-k]) / 2; returns |X[k]|^2.
// kk = (M - k) mod M.  For k == 0 *nyq = |X[n_fft/2]|^2 = (Re Z0 - Im Z0)^2 (purely real).
AT_MX_HD float untangle_power(int k, int kk, const float* z, const float* twn, float* nyq) {
    const float ar = z[2 * k], ai = z[2 * k + 1];
    const float br = z[2 * kk], bi = -z[2 * kk + 1];
    const float evr = 0.5f * (ar + br), evi = 0.5f * (ai + bi);
    const float dfr = 0.5f * (ar - br), dfi = 0.5f * (ai - bi);
    const float odr = dfi, odi = -dfr;
    const float wr = twn[2 * k], wi = twn[2 * k + 1];
    const float xr = evr + __builtin_fmaf(odr, wr, -(odi * wi));
    const float xi = evi + __builtin_fmaf(odr, wi, odi * wr);
    if (k == 0) {
        const float nq = ar - ai;
        *nyq = nq * nq;
    }
    return __builtin_fmaf(xr, xr, xi * xi);
}

// Z (M complex points, natural order) -> the M + 1 power bins pw[0 .. M]
template <typename Barrier>
AT_MX_HD void untangle_lanes(Lanes ln, int M, const float* z, const float* twn, float* pw, Barrier barrier) {
    for (int lane = ln.begin; lane < ln.end; lane++)
        for (int k = lane; k < M; k += 64) pw[k] = untangle_power(k, k ? M - k : 0, z, twn, pw + M);
    barrier();
}

// ---- host tables (double, rounded to fp32) --------------------------------------------------------------------------
// n x (cos, -sin) of 2 pi j / n
inline void twiddle_table(int n, float* out) {
    for (int j = 0; j < n; j++) {
        out[2 * j] = (float)std::cos(2.0 * M_PI * j / n);
        out[2 * j + 1] = (float)-std::sin(2.0 * M_PI * j / n);
    }
}
// n_fft/2 x (cos, -sin) of 2 pi k / n_fft: the untangling twiddles W_N^k, k < M
inline void untangle_table(int n_fft, float* out) {
    for (int k = 0; k < n_fft / 2; k++) {
        out[2 * k] = (float)std::cos(2.0 * M_PI * k / n_fft);
        out[2 * k + 1] = (float)-std::sin(2.0 * M_PI * k / n_fft);
    }
}
// in-place radix-2 FFT in double (host, tables only); n a power of two
inline void fft_double(std::vector<double>& re, std::vector<double>& im) {
    const int n = (int)re.size();
    for (int i = 1, j = 0; i < n; i++) {
        int bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) {
            std::swap(re[i], re[j]);
            std::swap(im[i], im[j]);
        }
    }
    for (int len = 2; len <= n; len <<= 1)
        for (int i = 0; i < n; i += len)
            for (int j = 0; j < len / 2; j++) {
                const double a = -2.0 * M_PI * j / len, wr = std::cos(a), wi = std::sin(a);
                const int p = i + j, q = i + j + len / 2;
                const double tr = re[q] * wr - im[q] * wi, ti = re[q] * wi + im[q] * wr;
                re[q] = re[p] - tr; im[q] = im[p] - ti;
                re[p] += tr; im[p] += ti;
            }
}
// chirp: M x w[n] = exp(-i pi n^2 / M) (n^2 reduced mod 2M in integers); bhat: P x FFT_P(b)/P with b[n] = b[P-n] =
// conj w[n] for n < M and zero between.
inline void bluestein_tables(int M, int P, float* chirp, float* bhat) {
    std::vector<double> re(P, 0.0), im(P, 0.0);
    for (int n = 0; n < M; n++) {
        const long e = ((long)n * n) % (2L * M);
        const double c = std::cos(M_PI * e / M), s = std::sin(M_PI * e / M);
        chirp[2 * n] = (float)c;
        chirp[2 * n + 1] = (float)-s;
        re[n] = c; im[n] = s;
        if (n) { re[P - n] = c; im[P - n] = s; }
    }
    fft_double(re, im);
    for (int i = 0; i < P; i++) {
        bhat[2 * i] = (float)(re[i] / P);
        bhat[2 * i + 1] = (float)(im[i] / P);
    }
}

}  // namespace lmx
