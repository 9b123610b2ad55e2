"""A numpy model of the resampler (csrc/resample.hip), exact to the bit, with no product or oracle code in it.

csrc/resample.hip states its arithmetic: output sample o = i*new + j of a clip is ONE fp32 fma chain over the taps of
phase j in ascending k, starting from +0, over the input window that starts at i*orig - width, zeros outside [0, L).
Every step rounds once, so the chain can be replayed on the host: `chain` does, and a kernel is then held to
np.array_equal on the bit patterns.  `dot64` is the yardstick beside it: the same dot product in float64 and the
textbook bound on what K roundings can do to it.

  taps(orig_freq, new_freq)           -> (float32 [new, K], orig, new, width)   the filter, K = 2*width + orig
  fma32(a, b, c)                      -> float32                                round(a*b + c), one rounding
  chain(w, orig_freq, new_freq, ...)  -> float32 [..., n]                       the kernel's bits
  dot64(w, orig_freq, new_freq, ...)  -> (float64 [..., n], bound [..., n])     value and |chain - value| bound

Beside them, what the CPU and the GPU tests share: the table of rate pairs (PAIRS, check_plan_record), the clip lengths
(lengths_for), the test clips with their references (clips, reference) and the impulse readout (impulse_response).
"""
import functools
import math

import numpy as np

LOWPASS_FILTER_WIDTH, ROLLOFF = 6, 0.99      # torchaudio.transforms.Resample's defaults
U32 = 2.0 ** -24                             # unit roundoff of float32

# The rate pairs the GPU tests run: (orig_freq, new_freq) -> (orig, new, width, K, TI, interleave).  TI is the tile (in
# input steps) that at_frontend_plan_host chooses, None where the filter does not fit the LDS segment and the plain
# one-thread-per-sample form runs; interleave is the tiled kernel's layout flag (new < 32).  Written down from the
# formulas, and asserted against the library's own plan by the tests (never trusted).
PAIRS = {
    (44100, 22050): (2, 1, 13, 28, 4080, True),
    (11025, 22050): (1, 2, 7, 15, 8176, True),
    (8000, 48000): (1, 6, 7, 15, 8176, True),
    (48000, 16000): (3, 1, 19, 41, 2716, True),
    (20000, 16000): (5, 4, 8, 21, 1632, True),
    (32000, 31000): (32, 31, 7, 46, 252, True),       # new = 31: the last interleaved layout
    (31000, 32000): (31, 32, 7, 45, 260, False),      # new = 32: the first adjacent one
    (48000, 22050): (320, 147, 14, 348, 24, False),
    (44100, 48000): (147, 160, 7, 161, 52, False),
    (16000, 22050): (320, 441, 7, 334, 24, False),
    (8000, 22050): (160, 441, 7, 174, 48, False),
    (32000, 22050): (640, 441, 9, 658, 12, False),
    (96000, 22050): (640, 147, 27, 694, 12, False),
    (44100, 16000): (441, 160, 17, 475, 16, False),
    (2044, 2043): (2044, 2043, 7, 2058, 4, False),    # four steps fit the segment: the smallest tile
    (2045, 2044): (2045, 2044, 7, 2059, None, False), # three fit: the plain form
    (2999, 3000): (2999, 3000, 7, 3013, None, False),
}


def check_plan_record(g, orig_freq, new_freq, tiled_mode, simple_mode):
    """Hold one PAIRS row to the group record `g` (fields orig, nw, width, K, mode, TI) that the library's plan writes
    for that pair; the caller passes the library's two mode constants.  The CPU and the GPU tests share it."""
    orig, new, width, K, TI, interleave = PAIRS[(orig_freq, new_freq)]
    assert (g["orig"], g["nw"], g["width"], g["K"]) == (orig, new, width, K), (orig_freq, new_freq)
    assert g["mode"] == (simple_mode if TI is None else tiled_mode), (orig_freq, new_freq)
    assert g["TI"] == (TI or 0), (orig_freq, new_freq)
    assert interleave == (TI is not None and new < 32), (orig_freq, new_freq)
    assert taps(orig_freq, new_freq)[0].shape == (new, K), (orig_freq, new_freq)


def reduced(orig_freq, new_freq):
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def out_length(L, orig_freq, new_freq):
    orig, new = reduced(orig_freq, new_freq)
    return -(-new * L // orig)                # ceil(new * L / orig)


@functools.lru_cache(maxsize=None)
def _taps(orig, new):
    base = min(orig, new) * ROLLOFF
    width = math.ceil(LOWPASS_FILTER_WIDTH * orig / base)
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx
    t = np.clip(t * base, -LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = np.cos(t * math.pi / LOWPASS_FILTER_WIDTH / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        kern = np.where(t == 0, 1.0, np.sin(t) / t)
    kern = (kern * window * (base / orig)).astype(np.float32)    # the one rounding to float32
    kern.setflags(write=False)
    return kern, width


def taps(orig_freq, new_freq):
    """torchaudio's sinc_interp_hann kernel as tests/test_resample_host.py::torch_resample states it, every operation
    in float64 in that order, rounded once to float32 -> (taps [new, K], orig, new, width)."""
    orig, new = reduced(orig_freq, new_freq)
    kern, width = _taps(orig, new)
    return kern, orig, new, width


def fma32(a, b, c):
    """round_to_float32(a*b + c) with ONE rounding, for float32 arrays (this Python has no math.fma).

    The float64 product of two float32 values is exact (48 bits).  The float64 sum p + c is not, and rounding it to
    float64 and then to float32 rounds twice: where the float64 sum lands on a float32 tie, the second rounding no
    longer knows on which side the exact value lay.  So the sum is computed with an error-free TwoSum (s + e == p + c
    exactly) and, where e != 0, s is moved to round-to-odd: of the two float64 neighbours of the exact sum, the one
    whose last mantissa bit is set.  A round-to-odd result with 53 bits is never a float32 tie or a float32 value unless
    the exact sum is, so the final rounding to float32 (24 bits, 53 >= 24 + 2) is the rounding of the exact sum."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float32) for v in (a, b, c)))
    return _fma32_f64(a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64))


def _fma32_f64(p, c):
    """fma32's second half: p the exact product and c the addend, both float64 arrays holding float32-representable
    values (p: products of two of them) -> float32."""
    shape = np.broadcast(p, c).shape
    p, c = np.atleast_1d(p), np.atleast_1d(c)
    s = np.atleast_1d(p + c)                  # an array of its own even for scalars: the bit edit below must land in it
    bb = s - p
    e = (p - (s - bb)) + (c - bb)             # TwoSum (Knuth): exact for any two doubles, no ordering needed
    # round to odd on the bits (sign and magnitude): where the sum is inexact, step the magnitude back if the rounding
    # went away from zero -- that is the truncated sum -- and set the last bit
    inexact = e != 0
    away = ((e < 0) != (s < 0)) & inexact
    bits = s.view(np.int64)
    assert np.shares_memory(bits, s)
    bits -= away
    bits |= inexact
    return s.astype(np.float32).reshape(shape)


def _gather(w, orig_freq, new_freq, outputs):
    """What chain and dot64 share -> (padded samples [B, *], first padded index per output, phase per output, taps,
    shape of the result)."""
    w = np.asarray(w, dtype=np.float32)
    lead = w.shape[:-1]
    x = w.reshape(-1, w.shape[-1])
    L = x.shape[1]
    t, orig, new, width = taps(orig_freq, new_freq)
    K = t.shape[1]
    n_out = out_length(L, orig_freq, new_freq)
    o = np.arange(n_out, dtype=np.int64) if outputs is None else np.asarray(outputs, dtype=np.int64).reshape(-1)
    assert o.size == 0 or (o.min() >= 0 and o.max() < n_out), "output index outside the clip"
    i, j = o // new, o % new
    hi = int(i.max()) * orig + K if o.size else K
    xp = np.zeros((x.shape[0], max(hi, width + L)), np.float32)      # xp[s + width] = x[s], +0 outside [0, L)
    xp[:, width: width + L] = x
    return xp, i * orig, j, t, lead + (o.size,)


def chain(w, orig_freq, new_freq, outputs=None):
    """The resampler's bits: for every output index o (all of them, or `outputs`), with i = o // new, j = o % new and
    s0 = i*orig - width: acc = +0, then for k = 0 .. K-1 in turn acc = fma32(x[s0 + k] or +0, taps[j][k], acc).
    w: [L] or [B, L] float32 -> float32 [n] or [B, n]."""
    xp, first, j, t, shape = _gather(w, orig_freq, new_freq, outputs)
    xp, t = xp.astype(np.float64), t.astype(np.float64)
    acc = np.zeros((xp.shape[0], first.size), np.float32)
    for k in range(t.shape[1]):
        acc = _fma32_f64(xp[:, first + k] * t[j, k][None, :], acc.astype(np.float64))
    return acc.reshape(shape)


def dot64(w, orig_freq, new_freq, outputs=None):
    """-> (values, bound): the float64 dot product of the float32 taps with the float32 samples, and the bound on
    |fl(.) - value| of a K-term fma recursion in float32 (Higham, Accuracy and Stability, section 3.1: every product
    passes through at most K roundings): gamma_K * sum_k |t_k| |x_k| with gamma_K = K*u / (1 - K*u), u = 2^-24.
    (The float64 dot itself is off by at most 2^-29 of that bound.)"""
    xp, first, j, t, shape = _gather(w, orig_freq, new_freq, outputs)
    K = t.shape[1]
    val = np.zeros((xp.shape[0], first.size), np.float64)
    mag = np.zeros_like(val)
    t64 = t.astype(np.float64)
    for k in range(K):
        p = xp[:, first + k].astype(np.float64) * t64[j, k][None, :]
        val += p
        mag += np.abs(p)
    return val.reshape(shape), (K * U32 / (1 - K * U32) * mag).reshape(shape)


def clips(orig_freq, new_freq, L, B=3):
    """The B test clips of length L at a pair (the same for every caller): white noise, a sine under a little noise,
    and noise whose level wanders over six decades, so that loud and very quiet samples share a tap window."""
    rng = np.random.default_rng([orig_freq, new_freq, L])
    w = rng.standard_normal((B, L))
    if B > 1:
        w[1] = 0.4 * np.sin(np.arange(L) * 0.037 + 1.0) + 0.05 * w[1]
    if B > 2:
        w[2] *= 10.0 ** rng.uniform(-3, 3, L)
    return w.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(orig_freq, new_freq, L):
    """-> (clips [3, L], chain, dot64 values, dot64 bound), computed once per process and read-only: the CPU tests that
    tie chain to dot64 and the GPU tests that hold the kernels to chain share them."""
    w = clips(orig_freq, new_freq, L)
    res = (w, chain(w, orig_freq, new_freq)) + dot64(w, orig_freq, new_freq)
    for a in res:
        a.setflags(write=False)
    return res


def impulse_response(L, p, orig_freq, new_freq):
    """What a clip that is zero except x[p] = 1 resamples to, read straight off the tap table: fma(0, t, acc) = acc and
    fma(1, t, +0) = t, so output i*new + j is taps[j][p - i*orig + width] where that index lies in [0, K) and +0
    elsewhere.  One exception: a tap at the clamped end of the window can round to -0.0 in float32, and 1 * -0 + +0 is
    +0.  No arithmetic otherwise."""
    t, orig, new, width = taps(orig_freq, new_freq)
    o = np.arange(out_length(L, orig_freq, new_freq), dtype=np.int64)
    i, j = o // new, o % new
    k = p - i * orig + width
    ok = (k >= 0) & (k < t.shape[1])
    out = np.zeros(o.size, np.float32)
    out[ok] = t[j[ok], k[ok]]
    return out + np.float32(0)                # (-0 + +0 = +0; every other value is unchanged)


def lengths_for(orig_freq, new_freq):
    """The clip lengths the kernels are run at, every one an edge of some branch (sorted, each once): clips shorter
    than the filter; lengths around one and two whole input steps (ceil(new*L/orig) on both sides of a step, a last
    step with fewer than `new` phases); a number of input steps n_i = ceil(L / orig) that is no multiple of the four
    accumulators a thread keeps; and, where the pair runs tiled, n_i = TI - 1, TI, TI + 1 (one step into a second
    tile) and 2*TI + 3."""
    orig, new, width, K, TI, _ = PAIRS[(orig_freq, new_freq)]
    Ls = {1, 2, width, width + 1, orig - 1, orig, orig + 1, 2 * orig + 1}
    steps = []
    if TI is not None:
        steps = [TI - 1, TI, TI + 1, 2 * TI + 3] + ([6] if TI > 8 else [])    # (TI = 4: TI - 1 and 2*TI + 3 are odd)
    for n, n_i in enumerate(steps):
        # any L in ((n_i - 1)*orig, n_i*orig] has n_i steps: take a different place inside the step each time
        Ls.add((n_i - 1) * orig + 1 + (n * 7 + orig // 2) % orig)
    return sorted(v for v in Ls if v >= 1)
