"""tests/resample_ref.py, the exact model the resampler's GPU tests compare bits with, held to things that need no GPU:
fma32 against exact rational arithmetic (on the ties where rounding twice goes wrong, too), the tap builder against the
library's host builder and the torch restatement, and the fma chain against the float64 dot product, its analytic
bound and the oracle -- so the new yardstick is tied to the existing one before a kernel is involved."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import oracle
import resample_ref as R
from audio_tokens_amd import _lib
from audio_tokens_amd.backend import HostHelpers
from test_resample_host import torch_resample

PAIRS = list(R.PAIRS)
CASES = [(o, n, L) for o, n in PAIRS for L in R.lengths_for(o, n)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- fma32 ---------------------------------------------------------------------------------------------------------------

def round_fraction_to_f32(x: Fraction) -> np.float32:
    """The float32 nearest to x, ties to the even mantissa, decided in rational arithmetic: float(x) is within one
    float32 ulp of the answer, so the answer is that value's float32 or one of its two neighbours."""
    c = np.float32(float(x))
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    dist = [abs(Fraction(float(v)) - x) for v in cands]
    best = min(dist)
    near = [v for v, d in zip(cands, dist) if d == best]
    if len(near) == 2:
        near = [v for v in near if int(v.view(np.uint32)) & 1 == 0]
    assert len(near) == 1
    return near[0]


def exact_fma(a, b, c):
    return np.array([round_fraction_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], np.float32)


def naive_fma(a, b, c):
    """The form that rounds twice: the exact float64 product, a float64 sum, then float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def test_fma32_matches_exact_arithmetic_on_random_triples():
    rng = np.random.default_rng(2024)
    n = 4000
    a, b, c = ((rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(np.float32) for _ in range(3))
    # a third of the addends nearly cancel the product (the sum then needs every bit of it), a few are zero
    near = slice(0, n // 3)
    c[near] = -(a[near] * b[near] * (1 + rng.integers(-4, 5, n // 3) * 2.0 ** -23)).astype(np.float32)
    c[n // 3: n // 3 + 50] = 0.0
    a[n // 3 + 50: n // 3 + 100] = 0.0
    assert np.array_equal(bits(R.fma32(a, b, c)), bits(exact_fma(a, b, c)))


def tie_triples():
    """Triples whose exact a*b + c lies a hair (below 2^-54 relative) to one side of a float32 tie, so that the float64
    sum is inexact and lands exactly ON the tie: a*b = 2^-24 * (1 + r * 2^-47) with 0 < |r| < 2^17, from integers
    a*b = 2^47 + r, against c = 1 + m * 2^-23, for which 1 + (m + 1/2) * 2^-23 is the tie.  Rounding the float64 sum to
    float32 breaks the tie towards the even mantissa whatever the sign of r: wrong for m even and r > 0, and for m odd
    and r < 0.  Scaled by powers of two and mirrored, so that every binade and both signs appear."""
    a, b, c = [], [], []
    x = 11863284                                        # just above sqrt(2^47)
    while len(a) < 64:
        x += 1
        y = (2 ** 47 + x // 2) // x
        r = x * y - 2 ** 47
        if r == 0 or abs(r) >= 2 ** 17 or not (2 ** 23 <= y < 2 ** 24):
            continue
        for m in (len(a) % 1000 * 2, len(a) % 1000 * 2 + 1):
            for sign in (1.0, -1.0):
                for e in (-9, 0, 14):
                    a.append(sign * x * 2.0 ** (-23 + e))
                    b.append(y * 2.0 ** -48)
                    c.append(sign * (1 + m * 2.0 ** -23) * 2.0 ** e)
    a, b, c = (np.array(v, np.float64) for v in (a, b, c))
    assert all(np.array_equal(v, v.astype(np.float32)) for v in (a, b, c))        # all are float32 values
    return a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)


def test_fma32_rounds_once_where_the_float64_sum_lands_on_a_float32_tie():
    a, b, c = tie_triples()
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    assert ((s.view(np.uint64) & 0x1FFFFFFF) == 0x10000000).all()                 # the float64 sum IS a float32 tie
    want = exact_fma(a, b, c)
    wrong = bits(naive_fma(a, b, c)) != bits(want)
    assert wrong.sum() >= len(a) // 4, "the constructed triples do not defeat double rounding: the check proves nothing"
    assert np.array_equal(bits(R.fma32(a, b, c)), bits(want))
    # one triple at a time, as numpy scalars, as 0-d arrays and as Python floats: the same single rounding, and a
    # result of the arguments' own shape
    for form in (lambda v: v, np.asarray, float):
        one = [R.fma32(form(x), form(y), form(z)) for x, y, z in zip(a, b, c)]
        assert all(r.shape == () and r.dtype == np.float32 for r in one)
        assert np.array_equal(bits(np.array(one, np.float32)), bits(want))
    assert R.fma32(a[:6].reshape(2, 3), b[:6].reshape(2, 3), c[0]).shape == (2, 3)


def test_fma32_readout_identities():
    """What the impulse test leans on: fma(1, t, +0) = t (but +0 for a tap of -0) and fma(0, t, acc) = acc, and +0
    stays +0."""
    t = np.array([0.3, -0.3, 1e-40, -1e-40, 2.0 ** -149, 0.0], np.float32)
    assert np.array_equal(bits(R.fma32(np.float32(1), t, np.float32(0))), bits(t))
    assert bits(R.fma32(np.float32(1), np.float32(-0.0), np.float32(0)))[0] == 0
    assert np.array_equal(bits(R.fma32(np.float32(0), np.float32(-0.25), t)), bits(t))
    assert bits(R.fma32(np.float32(0), np.float32(-0.25), np.float32(0)))[0] == 0


# ---- taps ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    return HostHelpers()


@pytest.mark.parametrize("orig_freq,new_freq", PAIRS)
def test_taps_match_the_host_builder_bit_for_bit(host, orig_freq, new_freq):
    want_taps, orig, new, width = host.resample_taps(orig_freq, new_freq)
    got = R.taps(orig_freq, new_freq)
    assert got[1:] == (orig, new, width) and got[0].dtype == np.float32
    assert (orig, new, width, 2 * width + orig) == R.PAIRS[(orig_freq, new_freq)][:4]
    assert got[0].shape == want_taps.shape and np.array_equal(bits(got[0]), bits(want_taps))


@pytest.mark.parametrize("orig_freq,new_freq", PAIRS)
def test_taps_match_torch_restatement(orig_freq, new_freq):
    _, kern = torch_resample(torch.zeros(1, 8), orig_freq, new_freq)
    got = R.taps(orig_freq, new_freq)[0]
    assert got.shape == tuple(kern.shape)
    np.testing.assert_allclose(got, kern.numpy(), rtol=0, atol=2e-7)


@pytest.mark.parametrize("orig_freq,new_freq", PAIRS)
def test_pair_table_is_what_the_plan_chooses(host, orig_freq, new_freq):
    """The table the GPU tests take their tile-crossing lengths from, against at_frontend_plan_host."""
    g = host.frontend_plan([1], [100], [orig_freq], new_freq, 64, 32)[2][0]
    R.check_plan_record(g, orig_freq, new_freq, _lib.AT_FRONTEND_TILED, _lib.AT_FRONTEND_SIMPLE)


# ---- chain and dot64 -----------------------------------------------------------------------------------------------------

def test_chain_is_the_scalar_recursion():
    """The vectorised chain against the definition written out with scalars, once with fma32 on scalars and once with
    every step rounded in rational arithmetic, at a pair with several phases, on every output of a short clip (all
    windows cut by the clip's ends) and a subset of a longer one."""
    for L, outputs in ((9, None), (700, [0, 1, 146, 147, 148, 300, 321])):
        w = R.clips(48000, 22050, L)[2]
        t, orig, new, width = R.taps(48000, 22050)
        idx = range(R.out_length(L, 48000, 22050)) if outputs is None else outputs
        want, exact = [], []
        for o in idx:
            i, j = divmod(o, new)
            acc = ex = np.float32(0)
            for k in range(t.shape[1]):
                s = i * orig - width + k
                x = w[s] if 0 <= s < L else np.float32(0)
                acc = R.fma32(x, t[j, k], acc)[()]
                ex = round_fraction_to_f32(Fraction(float(x)) * Fraction(float(t[j, k])) + Fraction(float(ex)))
            want.append(acc)
            exact.append(ex)
        got = bits(R.chain(w, 48000, 22050, outputs))
        assert np.array_equal(got, bits(np.array(exact, np.float32)))
        assert np.array_equal(got, bits(np.array(want, np.float32)))


@pytest.mark.parametrize("orig_freq,new_freq,L", CASES)
def test_chain_lies_within_the_bound_and_the_oracle_beside_it(orig_freq, new_freq, L):
    w, got, val, bound = R.reference(orig_freq, new_freq, L)
    assert got.shape == val.shape == (3, R.out_length(L, orig_freq, new_freq))
    assert (np.abs(got.astype(np.float64) - val) <= bound).all()
    # the oracle rounds a double dot product once: half an ulp of the value, beside what the bound already allows
    half_ulp = np.spacing(np.abs(val).astype(np.float32)).astype(np.float64) / 2
    for b in range(3):
        orc = oracle.resample(w[b], orig_freq, new_freq)
        assert orc.shape == val[b].shape
        assert (np.abs(orc.astype(np.float64) - val[b]) <= bound[b] + half_ulp[b]).all()


def test_impulse_response_is_the_chain_of_an_impulse():
    for orig_freq, new_freq in ((44100, 22050), (8000, 48000), (48000, 22050)):
        orig, new, width = R.PAIRS[(orig_freq, new_freq)][:3]
        L = 3 * orig + width
        for p in (0, 1, width, L // 2, L - 1):
            x = np.zeros(L, np.float32)
            x[p] = 1.0
            assert np.array_equal(bits(R.impulse_response(L, p, orig_freq, new_freq)), bits(R.chain(x, orig_freq, new_freq)))
