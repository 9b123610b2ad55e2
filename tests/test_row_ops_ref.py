"""The CPU references of the row and reduction kernels (tests/row_ops_ref.py) held to the libraries they model --
numpy's norm, torch's CPU min-max expression and conv1d, exact rational arithmetic, scipy's linregress -- and the edge
data shown to be edge data.  No GPU involved."""
import warnings
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest
import torch

from row_ops_ref import (CONV_CASES, CONV_NO_BIAS, FLT_MAX, HARD_ROW_KINDS, L2NORM_D_LADDER, MINMAX_CLIP_ELEMS,
                         MINMAX_CLIP_KINDS, TOKEN_STATS_K, bits, conv1d_mel_f64_shortcut, conv1d_mel_ref, conv_tie_data,
                         gaussian_rows, hard_rows, l2norm_ref, l2norm_rows_per_block, minmax_clip, minmax_ref, pairwise_sumsq_ref,
                         same_f32, serial_sumsq, token_histograms, token_stats_ref)

# every d of the GPU ladder, and both neighbours of 64
D_ALL = tuple(sorted(set(L2NORM_D_LADDER) | {63, 65}))


# ---- 1. l2norm --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", D_ALL)
def test_l2norm_ref_is_numpys_norm_bit_for_bit(d):
    rng = np.random.default_rng(d)
    x = np.concatenate([hard_rows(d, rng), hard_rows(d, rng),
                        (rng.standard_normal((5, d)) * np.array([1, 1e-22, 1e-30, 3e18, 1e19])[:, None]).astype(np.float32)])
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        want = x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-10)
    got = l2norm_ref(x)
    assert want.dtype == np.float32 and got.dtype == np.float32
    ok = same_f32(got, want)
    assert ok.all(), f"d={d}: rows {sorted(set(np.argwhere(~ok)[:, 0].tolist()))} differ"
    finite = np.isfinite(x).all(axis=1)
    assert np.array_equal(bits(got[finite]), bits(want[finite]))          # NaN leniency is not needed without NaN / Inf


def test_the_ladder_tells_numpys_tree_from_a_serial_sum():
    """Without this the d ladder would not pin the tree: at every d >= 8 some Gaussian row's pairwise sum of squares
    differs from the left-to-right one; below 8 the two are the same sum."""
    rng = np.random.default_rng(0)
    for d in D_ALL:
        x = rng.standard_normal((64, d)).astype(np.float32)
        differ = int((bits(pairwise_sumsq_ref(x)) != bits(serial_sumsq(x))).sum())
        if d < 8:
            assert differ == 0, d
        else:
            assert differ > 0, d


def test_rows_longer_than_numpys_buffer_are_summed_in_pieces_of_8192():
    """numpy's reduction hands its inner loop at most np.getbufsize() = 8192 elements at a time: at d = 8702 and 8703 the
    one pairwise tree over the whole row is NOT numpy's sum (the kernel computed that tree until these tests), at 16384
    the two are the same."""
    from row_ops_ref import _pairwise
    assert np.getbufsize() == 8192
    rng = np.random.default_rng(4)
    for d, expect in ((8192, False), (8702, True), (8703, True), (16384, False)):
        x = rng.standard_normal((64, d)).astype(np.float32)
        numpys = np.add.reduce(x * x, axis=1)
        assert np.array_equal(bits(pairwise_sumsq_ref(x)), bits(numpys)), d
        assert bool((bits(_pairwise(x * x)) != bits(numpys)).any()) == expect, d
        # ... and the 64 Gaussian rows the GPU test adds at every d show it in the normalised rows themselves
        g = gaussian_rows(64, d, np.random.default_rng(d))
        one_tree = g / (np.sqrt(_pairwise(g * g)) + np.float32(1e-10))[:, None]
        assert bool((bits(one_tree) != bits(l2norm_ref(g))).any()) == expect, d


def test_every_split_of_the_tree_shows_in_the_ladder():
    """Dropping the 'multiple of 8' rounding of the split changes the result at the d where n // 2 is no multiple of
    8 (134 .. 136, 270, 271, 542, 543, 1000 -- not 256, 264, 1280), which is why those d are in the ladder."""
    from row_ops_ref import _pairwise

    def unrounded(sq):
        n = sq.shape[-1]
        if n <= 128:
            return _pairwise(sq)
        return unrounded(sq[..., :n // 2]) + unrounded(sq[..., n // 2:])
    rng = np.random.default_rng(1)
    for d, expect in ((134, True), (135, True), (136, True), (270, True), (271, True), (542, True), (543, True), (1000, True),
                      (4099, True), (256, False), (264, True), (1280, False), (16384, False)):
        x = rng.standard_normal((64, d)).astype(np.float32)
        sq = x * x
        differ = bool((bits(_pairwise(sq)) != bits(unrounded(sq))).any())
        assert differ == expect, d


def test_hard_rows_are_what_they_say():
    rng = np.random.default_rng(2)
    for d in (1, 9, 129, 1280):
        x = hard_rows(d, rng)
        k = {name: x[i] for i, name in enumerate(HARD_ROW_KINDS)}
        ss = pairwise_sumsq_ref(x)
        s = dict(zip(HARD_ROW_KINDS, ss))
        tiny = np.finfo(np.float32).tiny
        assert not k["zeros"].any() and not np.signbit(k["zeros"]).any()
        assert not k["signed_zeros"].any() and (d < 9 or (np.signbit(k["signed_zeros"]).any() and not np.signbit(k["signed_zeros"]).all()))
        assert np.count_nonzero(k["single"]) == 1
        assert (np.abs(k["denormal"]) < tiny).all() and k["denormal"].any() and s["denormal"] == 0
        assert k["1e-30"].all() and s["1e-30"] == 0                      # squares underflow: the result is x / 1e-10
        assert 0 < s["1e-22"] < tiny                                     # the sum of squares is a denormal
        assert np.isfinite(k["3e18"] * k["3e18"]).all() and (s["3e18"] > 1e33 if d > 1 else True)   # squares fit, the sum
        assert np.isfinite(s["3e18"]) == (d <= 9)                                     # of a long row does not
        assert (np.abs(k["flt_max"]) == FLT_MAX).all() and np.isposinf(s["flt_max"])
        if d >= 9:
            assert np.isposinf(s["1e19"]) and np.isfinite(k["1e19"]).all()
        assert np.isposinf(k["pos_inf"]).sum() == 1 and np.isneginf(k["neg_inf"]).sum() == 1 and np.isnan(k["nan"]).sum() == 1
        out = l2norm_ref(x)
        o = {name: out[i] for i, name in enumerate(HARD_ROW_KINDS)}
        assert np.array_equal(bits(o["1e-30"]), bits(k["1e-30"] / np.float32(1e-10)))
        assert not o["flt_max"].any() and np.array_equal(np.signbit(o["flt_max"]), np.signbit(k["flt_max"]))
        assert np.isnan(o["nan"]).all() and np.isnan(o["pos_inf"]).sum() == 1


def test_rows_per_block_ladder():
    assert [l2norm_rows_per_block(d) for d in (1, 66, 67, 134, 135, 270, 271, 542, 543, 8702, 8703, 16384)] == \
        [256, 256, 128, 128, 64, 64, 32, 32, 16, 2, 1, 1]


# ---- 2. min-max -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", MINMAX_CLIP_ELEMS)
def test_minmax_ref_is_torchs_cpu_expression_bitwise(e):
    rng = np.random.default_rng(e)
    clips = np.stack([minmax_clip(kind, e, rng) for kind in MINMAX_CLIP_KINDS])
    got = minmax_ref(clips)
    for i, kind in enumerate(MINMAX_CLIP_KINDS):
        s = torch.from_numpy(clips[i])
        want = ((s - s.min()) / (s.max() - s.min())).numpy()
        assert same_f32(got[i], want).all(), (e, kind)
        assert not ((clips[i] == 0) & np.signbit(clips[i])).any() or not ((clips[i] == 0) & ~np.signbit(clips[i])).any()
    k = dict(zip(MINMAX_CLIP_KINDS, got))
    assert np.isnan(k["constant"]).all() and np.isnan(k["nan_first"]).all() and np.isnan(k["nan_last"]).all()
    assert np.isnan(k["neg_inf"]).all()
    if e >= 2:
        assert np.isnan(k["pos_inf"]).sum() == 1 and np.isnan(k["flt_max_pair"]).sum() == 1
        assert set(np.unique(k["two_valued"]).tolist()) == {0.0, 1.0}
        d = clips[MINMAX_CLIP_KINDS.index("denormal_range")]
        assert 0 < d.max() - d.min() < np.finfo(np.float32).tiny
    if e >= 63:
        assert np.isfinite(k["gaussian"]).all() and k["gaussian"].min() == 0 and k["gaussian"].max() == 1
        assert np.isfinite(k["denormal_range"]).all() and k["denormal_range"].max() == 1


# ---- 3. conv1d --------------------------------------------------------------------------------------------------------
def _round_f32(fr):
    """The float32 nearest to the Fraction fr, ties to even (finite results only)."""
    if fr == 0:
        return np.float32(0.0)
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    q = a / Fraction(2) ** (max(e, -126) - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    v = float(n) * 2.0 ** (max(e, -126) - 23)
    return np.float32(-v if fr < 0 else v)


def _conv_inputs(n_mels, nk, ks, n, kind, seed):
    rng = np.random.default_rng(seed)
    bias = (n_mels, nk, ks) != CONV_NO_BIAS
    if kind == "ties":
        return conv_tie_data(n, n_mels, nk, ks, rng, bias=bias)
    x = (rng.standard_normal((n, n_mels)) * 20 - 30).astype(np.float32)
    w = (rng.standard_normal((nk, ks)) / np.sqrt(ks)).astype(np.float32)
    return x, w, ((rng.standard_normal(nk)).astype(np.float32) if bias else None)


@pytest.mark.parametrize("kind", ["gaussian", "ties"])
@pytest.mark.parametrize("n_mels,nk,ks", CONV_CASES)
def test_conv1d_mel_ref_against_torch_and_exact_arithmetic(n_mels, nk, ks, kind):
    n = 3 if nk == 1024 else 30
    x, w, b = _conv_inputs(n_mels, nk, ks, n, kind, n_mels + nk + ks)
    pad = ks // 2
    got = conv1d_mel_ref(x, w, b, pad)
    assert got.shape == (n, n_mels * nk) and got.dtype == np.float32
    want = torch.nn.functional.conv1d(torch.from_numpy(x).unsqueeze(1), torch.from_numpy(w).unsqueeze(1),
                                      None if b is None else torch.from_numpy(b), padding=pad)
    want = want.transpose(1, 2).reshape(n, -1)
    if kind == "gaussian":        # (the dyadic data cancels over 2^+-24: torch's own order of the taps is not that close)
        assert torch.allclose(torch.from_numpy(got), want, rtol=1e-5, atol=1e-5)
    # exact: the chain in rational arithmetic, rounded to float32 once per tap, on sampled outputs
    rng = np.random.default_rng(7)
    picks = np.unique(rng.integers(0, got.size, 60))
    if kind == "ties":                                   # the planted outputs among them
        wrong = np.flatnonzero(bits(conv1d_mel_f64_shortcut(x, w, b, pad)).ravel() != bits(got).ravel())
        picks = np.unique(np.concatenate([picks, wrong[:20]]))
    for p in picks:
        row, f = divmod(int(p), n_mels * nk)
        m, j = divmod(f, nk)
        acc = np.float32(0.0) if b is None else b[j]
        for t in range(ks):
            mm = m + t - pad
            v = x[row, mm] if 0 <= mm < n_mels else np.float32(0.0)
            acc = _round_f32(Fraction(float(w[j, t])) * Fraction(float(v)) + Fraction(float(acc)))
        assert bits(acc) == bits(got[row, f]) or (acc == 0 and got[row, f] == 0), (row, m, j)


@pytest.mark.parametrize("n_mels,nk,ks", CONV_CASES)
def test_the_tie_data_trips_the_float64_shortcut(n_mels, nk, ks):
    """conv_tie_data is tie-prone in fact: the 'float64 multiply-add, then narrow' emulation that
    test_conv1d_mel_matches_torch used differs from the fmaf chain on it (and never on Gaussian data)."""
    for n in ((1, 3) if nk == 1024 else (1, 300)):
        x, w, b = _conv_inputs(n_mels, nk, ks, n, "ties", n)
        if n_mels == 1 and ks > 1:
            continue
        wrong = int((bits(conv1d_mel_f64_shortcut(x, w, b, ks // 2)) != bits(conv1d_mel_ref(x, w, b, ks // 2))).sum())
        print(f"({n_mels},{nk},{ks}) n={n}: the shortcut is wrong in {wrong} outputs")
        assert wrong > 0
    x, w, b = _conv_inputs(n_mels, nk, ks, 3 if nk == 1024 else 300, "gaussian", 5)
    assert np.array_equal(bits(conv1d_mel_f64_shortcut(x, w, b, ks // 2)), bits(conv1d_mel_ref(x, w, b, ks // 2)))


# ---- 4. token statistics ----------------------------------------------------------------------------------------------
def _recipe(counts):
    """spec_tokenizer.py's host recipe on the tokens a histogram stands for (scipy's linregress for the fit)."""
    from scipy import stats
    c = Counter({int(t): int(v) for t, v in enumerate(counts) if v > 0})
    ref = sorted(c.items(), key=lambda kv: (-kv[1], kv[0]))
    freq = np.array([v for _, v in ref], dtype=np.int64)
    out = dict(total=int(freq.sum()), unique=len(ref), tokens=[t for t, _ in ref], freq=freq)
    out["top_80"] = int(np.searchsorted(np.cumsum(freq) / freq.sum(), 0.8)) if len(ref) else 0
    s0, s1 = int(0.1 * len(freq)), int(0.9 * len(freq))
    out["n_fit"] = s1 - s0
    out["fit"] = None
    if s1 - s0 >= 2:
        lr, lf = np.log(np.arange(1, len(freq) + 1)), np.log(freq)
        out["fit"] = stats.linregress(lr[s0:s1], lf[s0:s1])
    return out


def _check_against_recipe(counts, name):
    got, ref = token_stats_ref(counts), _recipe(counts)
    u = ref["unique"]
    assert (got["total"], got["unique"], got["top_80"], got["n_fit"]) == (ref["total"], u, ref["top_80"], ref["n_fit"]), name
    assert got["sorted_tokens"][:u].tolist() == ref["tokens"] and np.array_equal(got["sorted_counts"][:u], ref["freq"]), name
    assert not got["sorted_counts"][u:].any() and np.all(np.diff(got["sorted_tokens"][u:]) > 0), name
    fit = ref["fit"]
    if fit is None:
        assert got["slope"] == 0 and got["intercept"] == 0 and got["r"] == 0, name
        return None
    if len(set(ref["freq"][int(0.1 * u):int(0.9 * u)].tolist())) == 1:           # all-equal counts: both sides are noise
        assert abs(fit.slope) < 1e-12 and abs(fit.rvalue) < 1e-12, (name, fit.slope, fit.rvalue)
        assert abs(got["slope"]) < 1e-12 and abs(got["r"]) < 1e-12, (name, got["slope"], got["r"])
        assert got["intercept"] == pytest.approx(fit.intercept, rel=1e-12)
        return max(abs(fit.slope), abs(got["slope"])), max(abs(fit.rvalue), abs(got["r"]))
    assert got["slope"] == pytest.approx(fit.slope, rel=1e-12), name
    assert got["intercept"] == pytest.approx(fit.intercept, rel=1e-12), name
    assert got["r"] == pytest.approx(fit.rvalue, rel=1e-12), name
    return None


@pytest.mark.parametrize("k", TOKEN_STATS_K)
def test_token_stats_ref_is_the_host_recipe(k):
    rng = np.random.default_rng(k)
    names = set()
    for name, counts in token_histograms(k, rng):
        assert counts.shape == (k,) and counts.dtype == np.int64
        _check_against_recipe(counts, name)
        names.add(name)
    assert len(names) == 8
    big = dict(token_histograms(k, rng))["above_2^32"]
    assert big.sum() > 2 ** 32 and big.max() > 2 ** 32


def test_token_stats_ref_at_every_unique_count_and_share_edge():
    rng = np.random.default_rng(3)
    for u in range(1, 41):
        for k in (64, 300):
            counts = np.zeros(k, np.int64)
            counts[rng.permutation(k)[:u]] = rng.integers(1, 1000, u)
            _check_against_recipe(counts, f"U={u}")
            assert token_stats_ref(counts)["n_fit"] == int(0.9 * u) - int(0.1 * u)
    for counts, top in (([4, 1], 0), ([3, 1], 1), ([5, 1], 0), ([8, 1, 1], 0), ([7, 1, 1], 1), ([9, 1, 1], 0)):
        _check_against_recipe(np.array(counts), str(counts))
        assert token_stats_ref(np.array(counts))["top_80"] == top, counts
    assert np.cumsum([4, 1])[0] / 5 == 0.8 and np.cumsum([8, 1, 1])[0] / 10 == 0.8      # the share lands on 0.8 exactly


def test_all_equal_counts_leave_only_rounding_noise_in_the_recipe():
    """All counts equal: the true slope and r are 0, and what the recipe and the reference return is rounding noise,
    below 1e-12 in magnitude (measured for m = 3 .. 20000: |slope| at most 1.8e-29, |r| at most 2.9e-15)."""
    worst = [0.0, 0.0]
    for m in (3, 10, 37, 255, 256, 257, 500, 1000, 8192, 20000):
        for c in (1, 37, 5_000_000_000):
            noise = _check_against_recipe(np.full(m, c, np.int64), f"m={m} c={c}")
            if noise is not None:
                worst = [max(worst[0], noise[0]), max(worst[1], noise[1])]
    print(f"all-equal counts: worst |slope| {worst[0]:.3g}, worst |r| {worst[1]:.3g}")
