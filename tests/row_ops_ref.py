"""CPU references of the row and reduction kernels (at_l2norm_rows_f32, at_minmax_scale_clips_f32, at_conv1d_mel_f32,
at_token_stats_f64) and the edge data their tests share, numpy only.  TEST ONLY.

Every reference is the kernel's stated contract written out step by step: numpy's pairwise float32 summation tree,
torch's float32 min-max expression, the fmaf chain of the convolution (spherical_ref.fma32 is an exact fmaf) and the
Counter / sorted / cumsum / searchsorted / linregress recipe of the token statistics.  tests/test_row_ops_ref.py holds
each of them to the library it models."""
import numpy as np

from spherical_ref import fma32

_F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_f32(got, want):
    """Elementwise: the same float32 bits, or a NaN on both sides.  (IEEE 754 leaves the sign and payload of a NaN that
    an operation produces to the implementation: 0 / 0 is 0xffc00000 on x86 and 0x7fc00000 on the GPU.)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


# ---- l2norm -----------------------------------------------------------------------------------------------------------
def _pairwise(sq):
    """sq [..., n] float32 squares -> [...] float32: numpy's pairwise_sum over the last axis, every step in float32."""
    n = sq.shape[-1]
    if n < 8:
        res = np.zeros(sq.shape[:-1], _F32)
        for i in range(n):
            res = res + sq[..., i]
        return res
    if n <= 128:
        r = sq[..., 0:8].copy()
        i = 8
        while i < n - (n % 8):
            r = r + sq[..., i:i + 8]
            i += 8
        res = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
        while i < n:
            res = res + sq[..., i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(sq[..., :n2]) + _pairwise(sq[..., n2:])


NUMPY_BUFSIZE = 8192          # np.getbufsize(): the most elements numpy's reduction hands its inner loop at a time


def pairwise_sumsq_ref(row):
    """Sum of squares of a float32 row (or of every row of [..., n]) as numpy's add.reduce(x * x) computes it: the
    pairwise tree over the row -- or, for a row longer than numpy's buffer of 8192 elements, the running sum, from
    +0, of the trees over its pieces of 8192 (the same as the one tree at n = 16384, not in between)."""
    row = np.asarray(row, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        sq = row * row
        out = np.zeros(sq.shape[:-1], _F32)
        for at in range(0, sq.shape[-1], NUMPY_BUFSIZE):
            out = out + _pairwise(sq[..., at:at + NUMPY_BUFSIZE])
    assert sq.dtype == np.float32 and out.dtype == np.float32
    return out


def serial_sumsq(x):
    """The plain left-to-right float32 sum of squares: what pairwise_sumsq_ref must NOT be for n >= 8."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        sq = x * x
        res = np.zeros(sq.shape[:-1], _F32)
        for i in range(sq.shape[-1]):
            res = res + sq[..., i]
    return res


def l2norm_ref(x):
    """x [n, d] float32 -> x / (sqrt(sumsq) + float32(1e-10)), all in float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        den = np.sqrt(pairwise_sumsq_ref(x)) + _F32(1e-10)
        out = x / den[:, None]
    assert den.dtype == np.float32 and out.dtype == np.float32
    return out


def l2norm_rows_per_block(d):
    """The kernel's rows per workgroup: 256, halved while R * (d + 2) floats exceed 68 KiB."""
    r = 256
    while r > 1 and r * (d + 2) * 4 > 68 * 1024:
        r >>= 1
    return r


L2NORM_D_LADDER = (1, 2, 7, 8, 9, 15, 16, 17, 64, 66, 67, 127, 128, 129, 134, 135, 136, 255, 256, 257, 264, 270, 271, 542,
                   543, 1000, 1280, 4099, 8702, 8703, 16384)

HARD_ROW_KINDS = ("gaussian", "zeros", "signed_zeros", "single", "denormal", "1e-30", "1e-22", "3e18", "1e19", "flt_max",
                  "pos_inf", "neg_inf", "nan")


def hard_rows(d, rng):
    """[len(HARD_ROW_KINDS), d] float32, one row per kind: Gaussian; all +0; mixed +-0; a single non-zero; denormals
    only; ~1e-30 (squares underflow to 0); ~1e-22 (squares denormal); ~3e18; ~1e19 and +-FLT_MAX (squares overflow);
    +inf, -inf and NaN at one position of a Gaussian row."""
    g = lambda: rng.standard_normal(d)
    pos = int(rng.integers(0, d))
    rows = []
    rows.append(g())
    rows.append(np.zeros(d))
    rows.append(np.where(rng.random(d) < 0.5, 0.0, -0.0))
    single = np.zeros(d)
    single[pos] = 3.7
    rows.append(single)
    rows.append(g() * 1e-40)
    rows.append(g() * 1e-30)
    rows.append(g() * 1e-22)
    rows.append(g() * 3e18)
    rows.append(g() * 1e19)
    rows.append(np.where(rng.random(d) < 0.5, FLT_MAX, -FLT_MAX).astype(np.float64))
    for bad in (np.inf, -np.inf, np.nan):
        r = g()
        r[pos] = bad
        rows.append(r)
    with np.errstate(over="ignore", under="ignore"):
        out = np.stack(rows).astype(np.float32)
    assert out.shape == (len(HARD_ROW_KINDS), d)
    return out


def gaussian_rows(n, d, rng):
    """[n, d] float32 Gaussian rows scaled by 1e-3 .. 1e2: the rows on which a wrong summation tree shows."""
    return (rng.standard_normal((n, d)) * rng.uniform(1e-3, 1e2, (n, 1))).astype(np.float32)


# ---- min-max ----------------------------------------------------------------------------------------------------------
def minmax_ref(clips):
    """clips [n, ...] float32 -> (x - lo) / (hi - lo) per clip in float32; np.min / np.max propagate NaN, as torch's."""
    clips = np.ascontiguousarray(clips, dtype=np.float32)
    flat = clips.reshape(clips.shape[0], -1)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        lo, hi = np.min(flat, axis=1, keepdims=True), np.max(flat, axis=1, keepdims=True)
        out = (flat - lo) / (hi - lo)
    assert out.dtype == np.float32
    return out.reshape(clips.shape)


MINMAX_CLIP_ELEMS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 64 * 345)
MINMAX_CLIP_KINDS = ("gaussian", "constant", "two_valued", "pos_inf", "neg_inf", "both_inf", "nan_first", "nan_last",
                     "flt_max_pair", "denormal_range")


def minmax_clip(kind, e, rng):
    """One clip of e float32 values of the given kind.  No clip holds both +0 and -0 (see test_gpu_row_ops.py)."""
    x = (rng.standard_normal(e) * 30 - 40).astype(np.float32)
    x[x == 0] = 1.0
    p, q = (int(v) for v in rng.permutation(e)[:2]) if e >= 2 else (0, 0)
    if kind == "constant":
        x[:] = _F32(-17.25)
    elif kind == "two_valued":
        x[:] = np.where(rng.random(e) < 0.5, _F32(2.5), _F32(-1.75))
        x[p], x[q] = 2.5, -1.75
    elif kind == "pos_inf":
        x[p] = np.inf
    elif kind == "neg_inf":
        x[p] = -np.inf
    elif kind == "both_inf":
        x[p], x[q] = np.inf, -np.inf
    elif kind == "nan_first":
        x[0] = np.nan
    elif kind == "nan_last":
        x[-1] = np.nan
    elif kind == "flt_max_pair":
        x[p], x[q] = FLT_MAX, -FLT_MAX
    elif kind == "denormal_range":                     # hi - lo (and every x - lo) is a denormal
        x = (_F32(1e-39) + rng.integers(0, 1 << 12, e).astype(np.float32) * _F32(1e-45)).astype(np.float32)
    else:
        assert kind == "gaussian"
    return x


# ---- conv1d along the mel axis ----------------------------------------------------------------------------------------
def conv1d_mel_ref(x, w, b, pad):
    """x [n, n_mels], w [nk, ks], b [nk] or None -> [n, n_mels * nk] float32 (feature = mel * nk + kernel): from the
    bias (or +0), the taps in ascending order, one exact fmaf each; a tap outside the row is multiplied by +0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    n, n_mels = x.shape
    nk, ks = w.shape
    assert 2 * pad == ks - 1
    xp = np.zeros((n, n_mels + 2 * pad), np.float32)
    xp[:, pad:pad + n_mels] = x
    start = np.zeros(nk, np.float32) if b is None else np.asarray(b, dtype=np.float32)
    acc = np.broadcast_to(start[None, None, :], (n, n_mels, nk)).copy()
    for t in range(ks):
        acc = fma32(w[None, None, :, t], xp[:, t:t + n_mels, None], acc)
    return acc.reshape(n, n_mels * nk)


def conv1d_mel_f64_shortcut(x, w, b, pad):
    """The emulation conv1d_mel_ref replaces: float64 multiply-add, then narrowed (two roundings, wrong on ties)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32).astype(np.float64)
    n, n_mels = x.shape
    nk, ks = w.shape
    xp = np.pad(x.astype(np.float64), ((0, 0), (pad, pad)))
    start = np.zeros(nk, np.float32) if b is None else np.asarray(b, dtype=np.float32)
    acc = np.broadcast_to(start[None, None, :], (n, n_mels, nk)).copy()
    for t in range(ks):
        acc = (acc.astype(np.float64) + xp[:, t:t + n_mels, None] * w[None, None, :, t]).astype(np.float32)
    return acc.reshape(n, n_mels * nk)


CONV_CASES = ((1, 1, 1), (2, 3, 5), (7, 1, 7), (64, 10, 3), (128, 10, 9), (64, 1024, 7), (40, 4, 5))   # (n_mels, nk, ks)
CONV_NO_BIAS = (40, 4, 5)
_W_TIE = _F32(1 - 2.0 ** -23)


def _dyadic(rng, shape):
    """Small integers times powers of two spread over 2^-12 .. 2^12."""
    return (rng.integers(-31, 32, shape) * 2.0 ** rng.integers(-12, 13, shape)).astype(np.float32)


def conv_tie_data(n, n_mels, nk, ks, rng, bias=True):
    """-> (x [n, n_mels], w [nk, ks], b [nk] or None): dyadic values on which every fmaf of the chain is decided by few
    bits, with ties planted for kernel 0.  A product of two small integers is too short to show a double rounding (the
    exact a * b + c must span more than 53 bits AND round to a float32 midpoint in float64, which takes a product of
    about 30 bits or more), so kernel 0's weights are 1 - 2^-23 and every third row (row 0 first) is a planted one:
      ks >= 2: the row is 0 but for x[m0] = 2^e * (1 + 2^-22) and x[m0 + 1] = +-2^(e-24) * (1 + 2^-23); kernel 0 starts
               from +0, reaches c = 2^e * (1 + 2^-23) (an odd significand) and then adds +-half_ulp(c) * (1 - 2^-46);
      ks == 1: the bias is c = 1.5 + 2^-23 and the row is +-2^-24 * (1 + 2^-23): again +-half_ulp * (1 - 2^-46).
    The correct result is c; the float64 sum lands exactly on the midpoint and narrows away from c when c is odd."""
    x, w = _dyadic(rng, (n, n_mels)), _dyadic(rng, (nk, ks))
    b = _dyadic(rng, nk) if bias else None
    w[0, :] = _W_TIE
    if ks == 1:
        assert bias
        b[0] = _F32(1.5 + 2.0 ** -23)
    elif bias:
        b[0] = 0.0
    for row in range(0, n, 3):
        sign = _F32(1.0 if rng.random() < 0.5 else -1.0)
        if ks == 1:
            x[row, :] = sign * _F32(2.0 ** -24 * (1 + 2.0 ** -23))
        elif n_mels >= 2:
            e = int(rng.integers(-12, 13))
            m0 = int(rng.integers(0, n_mels - 1))
            x[row, :] = 0.0
            x[row, m0] = _F32(2.0 ** e * (1 + 2.0 ** -22))
            x[row, m0 + 1] = sign * _F32(2.0 ** (e - 24) * (1 + 2.0 ** -23))
    return x, w, b


# ---- token statistics -------------------------------------------------------------------------------------------------
def token_stats_ref(counts):
    """counts int64 [k] -> dict(total, unique, top_80, n_fit, slope, intercept, r, sorted_counts [k], sorted_tokens [k]):
    order by (-count, token id); np.searchsorted(np.cumsum(freq) / total, 0.8) over the tokens that occur; the
    least-squares line through (ln rank, ln count) of ranks [int(0.1 U), int(0.9 U)) with scipy.stats.linregress'
    formulas in float64; fewer than 2 points: slope = intercept = r = 0."""
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.ndim == 1 and (counts >= 0).all()
    order = np.lexsort((np.arange(counts.size), -counts))
    sc = counts[order]
    freq = sc[sc > 0]
    total, unique = int(freq.sum()), int(freq.size)
    top_80 = int(np.searchsorted(np.cumsum(freq) / total, 0.8)) if unique else 0
    s0, s1 = int(0.1 * unique), int(0.9 * unique)
    slope = intercept = r = 0.0
    if s1 - s0 >= 2:
        lx, ly = np.log(np.arange(s0 + 1, s1 + 1, dtype=np.float64)), np.log(freq[s0:s1].astype(np.float64))
        xm, ym = lx.mean(), ly.mean()
        sxx, sxy, syy = np.mean((lx - xm) ** 2), np.mean((lx - xm) * (ly - ym)), np.mean((ly - ym) ** 2)
        slope = float(sxy / sxx)
        intercept = float(ym - slope * xm)
        r = float(min(1.0, max(-1.0, sxy / np.sqrt(sxx * syy)))) if sxx > 0 and syy > 0 else 0.0
    return dict(total=total, unique=unique, top_80=top_80, n_fit=s1 - s0, slope=slope, intercept=intercept, r=r,
                sorted_counts=sc, sorted_tokens=order.astype(np.int64))


TOKEN_STATS_K = (1, 2, 3, 10, 255, 256, 257, 500, 8192, 20000)


def token_histograms(k, rng):
    """-> list of (name, counts int64 [k]): the histogram ladder at vocabulary size k."""
    zipf = 1.0 / np.arange(1, k + 1) ** 1.1
    sample = np.bincount(rng.permutation(k)[rng.choice(k, size=max(50 * k, 1000), p=zipf / zipf.sum())], minlength=k)
    one = np.zeros(k, np.int64)
    one[int(rng.integers(0, k))] = 12345
    two = np.where(rng.random(k) < 0.4, 7, 3)
    runs = np.repeat(np.arange(1, k + 1), np.maximum(1, k // 7))[:k][rng.permutation(k)]   # runs of ~k/7 equal counts
    gaps = np.where(np.arange(k) % 3 == 1, 0, rng.integers(1, 50, k))
    out = [("zipf", sample), ("all_zero", np.zeros(k, np.int64)), ("one_nonzero", one), ("all_equal", np.full(k, 37)),
           ("two_values", two), ("tie_runs", runs), ("zeros_interleaved", gaps), ("above_2^32", sample * (5_000_000_000 // int(sample.max())))]
    return [(name, np.ascontiguousarray(c, dtype=np.int64)) for name, c in out]
