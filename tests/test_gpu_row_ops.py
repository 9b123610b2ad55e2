"""The row and reduction kernels at their shape and value edges: at_l2norm_rows_f32, at_minmax_scale_clips_f32,
at_conv1d_mel_f32, at_gather_rows_f32, at_sum_f32, at_any_nonfinite_f32, at_token_histogram_i64 and at_token_stats_f64
against the step-by-step references of tests/row_ops_ref.py (held to numpy / torch / scipy by tests/test_row_ops_ref.py).

Every comparison is on the uint32 / int64 bits unless a tolerance is stated.  One exception is made everywhere: where the
reference holds a NaN the kernel must hold a NaN, of any sign and payload -- IEEE 754 leaves both to the implementation
for a NaN that an operation produces (0 / 0 is 0xffc00000 on x86 and 0x7fc00000 on the GPU).  at_gather_rows_f32 copies
and is held to the payload too."""
import math

import numpy as np
import pytest
import torch

from device_rows import rows_one_float_off
from row_ops_ref import (CONV_CASES, CONV_NO_BIAS, FLT_MAX, L2NORM_D_LADDER, MINMAX_CLIP_ELEMS, MINMAX_CLIP_KINDS,
                         TOKEN_STATS_K, bits, conv1d_mel_ref, conv_tie_data, gaussian_rows, hard_rows, l2norm_ref,
                         l2norm_rows_per_block, minmax_clip, minmax_ref, same_f32, token_histograms, token_stats_ref)

pytestmark = pytest.mark.gpu


def _assert_same(got, want, what):
    ok = same_f32(got, want)
    if not ok.all():
        at = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} values differ, first at {at}: got {got[at]!r} "
                             f"({bits(got)[at]:#010x}) want {want[at]!r} ({bits(want)[at]:#010x})")


# ---- l2norm -----------------------------------------------------------------------------------------------------------
def _ladder_rows(n, d, rng):
    """n rows that walk the value ladder (a fresh draw of hard_rows per 13 rows), Gaussian first."""
    reps = -(-n // 13)
    return np.concatenate([hard_rows(d, rng) for _ in range(reps)])[:n]


@pytest.mark.parametrize("d", L2NORM_D_LADDER)
def test_l2norm_rows_at_every_tree_and_block_geometry(be, d):
    """numpy's bits at every d where its summation tree or the kernel's rows per workgroup R change (8 / 128 / every
    halving; R * (d + 2) floats <= 68 KiB; rows longer than numpy's buffer of 8192), n around R, every row kind of the
    value ladder at every d, and in place.  (d = 8702 and 8703 found the kernel summing the whole row with one tree
    where numpy sums pieces of 8192.)"""
    rng = np.random.default_rng(d)
    R = l2norm_rows_per_block(d)
    ns = sorted({n for n in (1, R - 1, R, R + 1, 2 * R + 3, 13) if n >= 1})
    # (few rows of the value ladder can tell two trees apart, and a sum that is one ulp off shows in about one row's
    # output in seven: 64 Gaussian rows of mixed scale go with every d -- tests/test_row_ops_ref.py counts on them)
    batches = [_ladder_rows(n, d, rng) for n in ns] + [gaussian_rows(64, d, rng)]
    for x in batches:
        n = len(x)
        want = l2norm_ref(x)
        xt = be._f32(x)
        got = be.l2norm_rows(xt).cpu().numpy()
        _assert_same(got, want, f"d={d} n={n} (R={R})")
        assert np.array_equal(bits(xt.cpu().numpy()), bits(x))                   # the input is left alone
        inplace = be.l2norm_rows(xt, out=xt)
        assert inplace.data_ptr() == xt.data_ptr()
        assert np.array_equal(bits(inplace.cpu().numpy()), bits(got)), f"d={d} n={n}: in place differs"


@pytest.mark.parametrize("d", [67, 1280])
def test_l2norm_rows_one_float_off_alignment(be, d):
    rng = np.random.default_rng(d)
    x = _ladder_rows(2 * l2norm_rows_per_block(d) + 3, d, rng)
    xu = rows_one_float_off(x, be.device)
    got = be.l2norm_rows(xu).cpu().numpy()
    _assert_same(got, l2norm_ref(x), f"d={d} unaligned")
    assert np.array_equal(bits(got), bits(be.l2norm_rows(be._f32(x)).cpu().numpy()))


def test_l2norm_rows_refuses_d_above_16384(be):
    from audio_tokens_amd import _lib
    x = torch.ones(2, 16385, device=be.device)
    with pytest.raises(_lib.NativeError, match="d=16385 not supported"):
        be.l2norm_rows(x)
    y = be.l2norm_rows(x[:, :16384].contiguous()).cpu().numpy()                  # the context works afterwards
    _assert_same(y, l2norm_ref(np.ones((2, 16384), np.float32)), "after the refusal")


# ---- min-max ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", MINMAX_CLIP_ELEMS)
def test_minmax_scale_clips_at_every_length_and_clip_kind(be, e):
    """(x - lo) / (hi - lo) with float32 operations, one 1024-thread workgroup per clip: clips shorter than the workgroup
    (idle lanes carry +-inf into the reduction), one element more than a full pass, and every clip kind alone (n_clips =
    1) and between two others (n_clips = 3).  No clip holds both +0 and -0: torch's own min / max pick either of the
    two by position, so the sign of a zero result is not defined by the reference."""
    rng = np.random.default_rng(e)
    for kind in MINMAX_CLIP_KINDS:
        clip = minmax_clip(kind, e, rng)
        for clips in (clip[None], np.stack([minmax_clip("gaussian", e, rng), clip, minmax_clip("two_valued", e, rng)])):
            want = minmax_ref(clips)
            t = be.from_host(clips)
            got = be.minmax_scale_clips(t)
            assert got.data_ptr() == t.data_ptr()
            _assert_same(got.cpu().numpy(), want, f"e={e} {kind} n_clips={len(clips)}")


def test_minmax_scale_clips_on_a_grid_wider_than_65535(be):
    rng = np.random.default_rng(5)
    clips = (rng.standard_normal((70000, 5)) * 30 - 40).astype(np.float32)
    for i, kind in ((0, "constant"), (65535, "nan_first"), (65536, "pos_inf"), (69999, "flt_max_pair"), (40000, "denormal_range")):
        clips[i] = minmax_clip(kind, 5, rng)
    got = be.minmax_scale_clips(be.from_host(clips)).cpu().numpy()
    _assert_same(got, minmax_ref(clips), "70000 clips of 5")


# ---- conv1d -----------------------------------------------------------------------------------------------------------
def _conv_data(n_mels, nk, ks, n, kind, rng):
    bias = (n_mels, nk, ks) != CONV_NO_BIAS
    if kind == "ties":
        return conv_tie_data(n, n_mels, nk, ks, rng, bias=bias)
    x = (rng.standard_normal((n, n_mels)) * 20 - 30).astype(np.float32)
    w = (rng.standard_normal((nk, ks)) / np.sqrt(ks)).astype(np.float32)
    return x, w, (rng.standard_normal(nk).astype(np.float32) if bias else None)


def _conv_device(be, x, w, b, ks):
    wt = torch.from_numpy(w).reshape(w.shape[0], 1, ks)
    return be.conv1d_mel(x, wt, None if b is None else torch.from_numpy(b), padding=ks // 2).cpu().numpy()


@pytest.mark.parametrize("kind", ["gaussian", "ties"])
@pytest.mark.parametrize("n_mels,nk,ks", CONV_CASES)
def test_conv1d_mel_is_the_fmaf_chain(be, n_mels, nk, ks, kind):
    """Bias (or +0), then the taps in ascending order, one fmaf each, bit for bit: n_mels below, at and above the kernel
    size, weights plus biases of exactly 32 KiB ((64, 1024, 7)), no bias ((40, 4, 5)); Gaussian data, and dyadic data
    with planted ties on which a float64 multiply-add rounded twice is wrong (tests/test_row_ops_ref.py shows it) --
    as is a separate multiply and add.  Gaussian data also within torch's 1e-5 of conv1d on the CPU."""
    rng = np.random.default_rng(n_mels + nk + ks)
    for n in ((1, 3) if nk == 1024 else (1, 300)):
        x, w, b = _conv_data(n_mels, nk, ks, n, kind, rng)
        got = _conv_device(be, x, w, b, ks)
        want = conv1d_mel_ref(x, w, b, ks // 2)
        assert got.shape == want.shape
        _assert_same(got, want, f"({n_mels},{nk},{ks}) n={n} {kind}")
        if kind == "gaussian":
            tw = torch.nn.functional.conv1d(torch.from_numpy(x).unsqueeze(1), torch.from_numpy(w).unsqueeze(1),
                                            None if b is None else torch.from_numpy(b), padding=ks // 2)
            assert torch.allclose(torch.from_numpy(got), tw.transpose(1, 2).reshape(n, -1), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kind", ["gaussian", "ties"])
def test_conv1d_mel_past_the_capped_grid(be, kind):
    """n = 7000 at (64, 10, 3): 4.48 M outputs, more than the 8 * 256 * 2048 one pass of the capped grid covers, so
    workgroups loop.  The rows are 7000 draws (with repeats, in random order) from 300 rows whose reference is computed
    once: every output of a row depends on that row alone."""
    n_mels, nk, ks, n = 64, 10, 3, 7000
    assert n * n_mels * nk > 8 * 256 * 2048
    rng = np.random.default_rng(9)
    base, w, b = _conv_data(n_mels, nk, ks, 300, kind, rng)
    pick = rng.integers(0, 300, n)
    got = _conv_device(be, base[pick], w, b, ks)
    _assert_same(got, conv1d_mel_ref(base, w, b, ks // 2)[pick], f"n={n} {kind}")


def test_conv1d_mel_refuses_more_than_32_kib_of_weights(be):
    from audio_tokens_amd import _lib
    x = torch.zeros(3, 64)
    with pytest.raises(_lib.NativeError, match="too many weights"):
        be.conv1d_mel(x, torch.zeros(1025, 1, 7), torch.zeros(1025), padding=3)
    assert not be.conv1d_mel(x, torch.zeros(1024, 1, 7), torch.zeros(1024), padding=3).any()


# ---- gather -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 4, 7, 64, 128, 640])
def test_gather_rows_copies_every_bit_pattern_at_every_index_shape(be, d):
    """Rows of random uint32 patterns (NaN payloads, -0, denormals) must arrive bit for bit: indices with repeats, all
    equal, 0 and n - 1 alone, descending; m in {0, 1, n, 3n}."""
    rng = np.random.default_rng(d)
    n = 257
    u = rng.integers(0, 2 ** 32, (n, d), dtype=np.uint64).astype(np.uint32)
    u[5, :] = 0x80000000                                                         # -0
    u[6, :] = 0x7fa00001 if d < 2 else np.where(np.arange(d) % 2 == 0, 0x7fa00001, 0xffc12345)   # NaNs with payloads
    u[7, :] = 0x00000001                                                         # the smallest denormal
    x = torch.from_numpy(u.view(np.int32)).to(be.device).view(torch.float32)
    cases = {"repeats_3n": rng.integers(0, n, 3 * n), "repeats_n": rng.integers(0, n, n), "all_equal": np.full(n, 6),
             "first": np.array([0]), "last": np.array([n - 1]), "ends": np.array([0, n - 1, n - 1, 0]),
             "descending": np.arange(n - 1, -1, -1), "descending_3n": np.repeat(np.arange(n - 1, -1, -1), 3),
             "empty": np.zeros(0, np.int64), "special_rows": np.array([5, 6, 7, 6, 5])}
    for name, idx in cases.items():
        got = be.gather_rows(x, idx.astype(np.int32))
        assert tuple(got.shape) == (len(idx), d), name
        assert np.array_equal(got.view(torch.int32).cpu().numpy().view(np.uint32), u[idx]), f"d={d} {name}"


# ---- sum --------------------------------------------------------------------------------------------------------------
SUM_N = (0, 1, 255, 256, 257, 1023, 1024, 1025, 262144, 262145, 2 ** 22, 2 ** 22 + 1)


def _sum_data(kind, n, rng):
    if kind == "uniform":
        return rng.random(n).astype(np.float32)
    if kind == "cancelling":                      # 1e8, 1, -1e8, 1, ...: a float accumulator loses every 1
        v = np.ones(n, np.float32)
        big = np.arange(0, n, 2)
        big = big[:len(big) - len(big) % 2]        # as many +1e8 as -1e8
        v[big] = np.where(np.arange(len(big)) % 2 == 0, 1e8, -1e8).astype(np.float32)
        return v
    if kind == "denormals":
        return (rng.integers(-(1 << 20), 1 << 20, n).astype(np.float32) * np.float32(1e-45)).astype(np.float32)
    v = rng.standard_normal(n).astype(np.float32)
    if n:
        p = rng.permutation(n)
        if kind == "one_inf":
            v[p[0]] = np.inf
        elif kind == "both_inf":
            v[p[0]] = np.inf
            v[p[-1]] = -np.inf
        elif kind == "one_nan":
            v[p[0]] = np.nan
    return v


@pytest.mark.parametrize("kind", ["uniform", "cancelling", "denormals", "one_inf", "both_inf", "one_nan"])
def test_sum_f64_within_the_bound_of_double_summation(be, kind):
    """at_sum_f32 adds in double, in a fixed tree: |got - exact| <= n * 2^-53 * sum |v|, the standard bound of
    recursive summation of doubles in ANY order (exact = math.fsum), at the sizes where the grid changes (one workgroup
    per 1024 values, capped at 256 workgroups up to 2^22 values and at 1024 above).  Non-finite values give what IEEE
    addition gives.  Three calls in a row return the same bits.  Worst ratio |got - exact| / bound seen on the MI355X:
    4.8e-7 for uniform data, 0 for the cancelling and the denormal data (their sums are exact in double)."""
    rng = np.random.default_rng(len(kind))
    worst = 0.0
    for n in SUM_N:
        v = _sum_data(kind, n, rng)
        vt = be.from_host(v)
        got = be.sum_f64(vt).item()
        for _ in range(2):
            again = be.sum_f64(vt).item()
            assert np.float64(again).view(np.uint64) == np.float64(got).view(np.uint64), (kind, n)
        if kind == "one_inf" and n >= 1:
            assert got == math.inf, (n, got)
        elif kind == "both_inf" and n >= 2:
            assert math.isnan(got), (n, got)
        elif kind == "one_nan" and n >= 1:
            assert math.isnan(got), (n, got)
        else:
            finite = v[np.isfinite(v)] if kind in ("one_inf", "both_inf", "one_nan") else v
            if finite.size != v.size:
                assert not math.isfinite(got)
                continue
            exact = math.fsum(v.astype(np.float64).tolist())
            bound = n * 2.0 ** -53 * math.fsum(np.abs(v).astype(np.float64).tolist())
            err = abs(got - exact)
            assert err <= bound, (kind, n, got, exact, err, bound)
            if bound > 0:
                worst = max(worst, err / bound)
            if kind == "cancelling":
                assert got == exact and exact >= n // 2
    print(f"at_sum_f32 {kind}: worst |got - exact| / (n 2^-53 sum|v|) = {worst:.3g}")


# ---- non-finite scan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 524288, 524289, 3000001])
def test_any_nonfinite_finds_one_bad_value_anywhere(be, n):
    """2048 workgroups of 256 threads are one full grid (524288 values): one bad value at the first, middle and last
    position and on either side of the grid's end; +inf, -inf, NaN and a negative signalling NaN whose payload is one
    bit; the largest finite values, denormals and -0 are not flagged; a clean call after a flagged one returns 0."""
    rng = np.random.default_rng(n)
    clean = rng.standard_normal(n).astype(np.float32)
    t = be.from_host(clean)
    ti = t.view(torch.int32)
    assert not be.any_nonfinite(t)
    bad_bits = {"+inf": 0x7f800000, "-inf": 0xff800000 - (1 << 32), "nan": 0x7fc00000, "-snan": 0xff800001 - (1 << 32)}
    for pos in sorted({p for p in (0, n // 2, n - 1, 524287, 524288) if p < n}):
        keep = int(ti[pos].item())
        for name, pattern in bad_bits.items():
            ti[pos] = pattern
            assert be.any_nonfinite(t), (n, pos, name)
            ti[pos] = keep
            assert not be.any_nonfinite(t), (n, pos, name, "clean again")
    for value in (FLT_MAX, -FLT_MAX, 1e-45, -1e-40, -0.0):
        assert not be.any_nonfinite(be.from_host(np.full(n, value, np.float32))), (n, value)


# ---- token histogram --------------------------------------------------------------------------------------------------
HIST_N = (0, 1, 4095, 4096, 4097, 1024 * 4096 + 1)


@pytest.mark.parametrize("k", [1, 2, 255, 256, 257, 16384, 16385, 20000])
def test_token_histogram_at_the_lds_switch_and_with_ids_out_of_range(be, k):
    """np.bincount of the ids inside [0, k): k on either side of the 256 threads and of the LDS / global switch (16384 |
    16385), n on either side of one workgroup's 4096 ids and past the 1024-workgroup cap; uniform ids, one token only,
    and ids outside the range mixed in -- -1, -2^63, k, k + 7, 2^31, 2^32, 2^32 + 3, 2^63 - 1: none may be counted, and
    none may alias onto a bin (2^32 + 3 is bin 3 to a 32-bit compare)."""
    rng = np.random.default_rng(k)
    outside = np.array([-1, -2 ** 63, k, k + 7, 2 ** 31, 2 ** 32, 2 ** 32 + 3, 2 ** 63 - 1], dtype=np.int64)
    for n in HIST_N:
        uniform = rng.integers(0, k, n).astype(np.int64)
        mixed = uniform.copy()
        if n:
            at = rng.permutation(n)[:max(8, n // 4)]
            mixed[at] = outside[np.arange(len(at)) % 8]
        cases = [("uniform", uniform), ("one_token", np.full(n, k - 1, np.int64)), ("mixed", mixed)]
        if n == 1:
            cases += [(f"outside {v}", np.array([v], np.int64)) for v in outside]
        for name, ids in cases:
            got = be.token_histogram(ids, k).cpu().numpy()
            inside = ids[(ids >= 0) & (ids < k)]
            want = np.bincount(inside, minlength=k).astype(np.int64)
            assert got.dtype == np.int64 and np.array_equal(got, want), f"k={k} n={n} {name}"


# ---- token statistics -------------------------------------------------------------------------------------------------
def _device_stats(be, counts):
    sc, stok, st = be.token_stats(be.from_host(np.ascontiguousarray(counts, dtype=np.int64)))
    st = st.cpu().numpy()
    return dict(total=int(st[0]), unique=int(st[1]), top_80=int(st[2]), slope=float(st[3]), intercept=float(st[4]),
                r=float(st[5]), n_fit=int(st[6]), sorted_counts=sc.cpu().numpy(), sorted_tokens=stok.cpu().numpy())


def _check_stats(be, counts, name):
    """Integers exact; slope, intercept and r to rel 1e-10 (the tolerance of
    test_token_statistics_on_the_device_match_numpy_and_scipy) where the reference is >= 1e-9 in magnitude, else both
    sides are rounding noise of an exact 0 and the device value must stay below 1e-9.  -> the device's dict."""
    got, ref = _device_stats(be, counts), token_stats_ref(counts)
    for key in ("total", "unique", "top_80", "n_fit"):
        assert got[key] == ref[key], f"{name}: {key} {got[key]} != {ref[key]}"
    assert np.array_equal(got["sorted_counts"], ref["sorted_counts"]), name
    assert np.array_equal(got["sorted_tokens"].astype(np.int64), ref["sorted_tokens"]), f"{name}: order is not (-count, id)"
    for key in ("slope", "intercept", "r"):
        if abs(ref[key]) >= 1e-9:
            assert got[key] == pytest.approx(ref[key], rel=1e-10), f"{name}: {key}"
        else:
            assert abs(got[key]) <= 1e-9, f"{name}: {key} {got[key]} (reference {ref[key]})"
    if ref["n_fit"] < 2:
        assert got["slope"] == 0 and got["intercept"] == 0 and got["r"] == 0, name
    return got


@pytest.mark.parametrize("k", TOKEN_STATS_K)
def test_token_stats_on_the_histogram_ladder(be, k):
    """k below, at and above the kernel's 256 threads (and no multiple of them); a Zipf sample, all zero, one non-zero,
    all equal, two distinct values, long runs of ties under permuted token ids, zeros interleaved, counts near 5e9."""
    rng = np.random.default_rng(k)
    for name, counts in token_histograms(k, rng):
        _check_stats(be, counts, f"k={k} {name}")


def test_token_stats_at_every_unique_count_and_on_the_80_percent_edge(be):
    """U = 1 .. 40 tokens that occur among k = 64 and k = 300: n_fit = int(0.9 U) - int(0.1 U) exactly (the fit is
    defined as 0 below two points); cumulative shares that land on 0.8 exactly ([4, 1], [8, 1, 1]: searchsorted's
    'left' counts the ranks strictly below) and one count to either side."""
    rng = np.random.default_rng(3)
    for u in range(1, 41):
        for k in (64, 300):
            counts = np.zeros(k, np.int64)
            counts[rng.permutation(k)[:u]] = rng.integers(1, 1000, u)
            got = _check_stats(be, counts, f"U={u} k={k}")
            assert got["n_fit"] == int(0.9 * u) - int(0.1 * u) and got["unique"] == u
    for counts, top in (([4, 1], 0), ([3, 1], 1), ([5, 1], 0), ([8, 1, 1], 0), ([7, 1, 1], 1), ([9, 1, 1], 0)):
        for pad in (0, 300):
            got = _check_stats(be, np.array(counts + [0] * pad), f"{counts} + {pad} zeros")
            assert got["top_80"] == top, (counts, pad, got["top_80"])


def test_token_stats_of_all_equal_counts_is_zero_up_to_rounding_noise(be):
    """All counts equal: slope and r are 0 in exact arithmetic and rounding noise of order m * 2^-53 on both sides
    (the reference's own stays below 1e-12: tests/test_row_ops_ref.py), so |slope| and |r| <= 1e-9, and the intercept
    is ln(count) to rel 1e-10.  Largest device values seen on the MI355X: |slope| 1.4e-29, |r| 2.2e-15."""
    worst = [0.0, 0.0]
    for m in (3, 10, 37, 255, 256, 257, 500, 1000, 8192, 20000):
        for c in (1, 37, 5_000_000_000):
            got = _check_stats(be, np.full(m, c, np.int64), f"m={m} c={c}")
            if got["n_fit"] >= 2:
                assert abs(got["slope"]) <= 1e-9 and abs(got["r"]) <= 1e-9, (m, c, got["slope"], got["r"])
                if c > 1:
                    assert got["intercept"] == pytest.approx(math.log(c), rel=1e-10), (m, c)
                else:
                    assert abs(got["intercept"]) <= 1e-9, (m, c)
                worst = [max(worst[0], abs(got["slope"])), max(worst[1], abs(got["r"]))]
    print(f"all-equal counts on the device: worst |slope| {worst[0]:.3g}, worst |r| {worst[1]:.3g}")
