"""CPU checks of the ROC AUC / threshold-metric yardstick (tests/roc_auc_ref.py) against sklearn, of a numpy model of
the kernel's tile / carry scheme against the yardstick, and of the library's exports.

Bound against sklearn: |roc_auc_score - auc| <= (G + 10) 2^-53, G the number of groups of equal scores."""
import functools
import math
import warnings
from fractions import Fraction

import numpy as np
import pytest

from roc_auc_ref import (CASES, f1_hamming_ref, make_case, roc_auc_column, roc_auc_ref, sklearn_auc_bound,
                         threshold_counts_ref)


@functools.lru_cache(maxsize=None)
def _case(name):
    labels, scores = make_case(name)
    ref = roc_auc_ref(labels, scores)
    for a in (labels, scores, ref["auc"], ref["n_pos"]):
        a.setflags(write=False)
    return labels, scores, ref


@pytest.mark.parametrize("name", CASES)
def test_yardstick_matches_sklearn_roc_auc(name):
    sk = pytest.importorskip("sklearn.metrics")
    labels, scores, ref = _case(name)
    bounds = sklearn_auc_bound(ref["groups"])
    worst = 0.0
    for j in range(0, labels.shape[1], 7 if labels.shape[1] > 100 else 1):   # (every 7th of 543 classes: time)
        if ref["exact"][j] is None:
            assert np.isnan(ref["auc"][j])
            with warnings.catch_warnings():          # sklearn raises ValueError here, or (1.7 on) warns and gives NaN
                warnings.simplefilter("ignore")
                try:
                    assert np.isnan(sk.roc_auc_score(labels[:, j], scores[:, j]))
                except ValueError as e:
                    assert "Only one class present" in str(e)
            continue
        theirs = sk.roc_auc_score(labels[:, j], scores[:, j])
        # the yardstick's float is the exact ratio rounded three times (two conversions, one division)
        assert abs(Fraction(float(ref["auc"][j])) - ref["exact"][j]) <= Fraction(4, 2 ** 53)
        err = abs(Fraction(theirs) - ref["exact"][j])
        worst = max(worst, float(err) / bounds[j])
        assert err <= Fraction(float(bounds[j])), (name, j, theirs, ref["auc"][j], int(ref["groups"][j]))
    print(f"{name}: sklearn within {worst:.3f} of the bound")


@pytest.mark.parametrize("name", ["3x2_signed_zeros", "65x7", "257x543", "300x4_extremes", "500x6_degenerate"])
@pytest.mark.parametrize("threshold", [0.2, 0.0, 0.5])
def test_yardstick_matches_sklearn_threshold_metrics(name, threshold):
    sk = pytest.importorskip("sklearn.metrics")
    labels, scores, _ = _case(name)
    n = labels.shape[0]
    pred = scores > threshold
    ref = f1_hamming_ref(threshold_counts_ref(labels, scores, threshold), n)
    tol = 2.0 ** -52
    assert abs(ref["micro"] - sk.f1_score(labels, pred, average="micro", zero_division=0)) <= tol
    assert abs(ref["macro"] - sk.f1_score(labels, pred, average="macro", zero_division=0)) <= tol
    assert abs(ref["hamming"] - sk.hamming_loss(labels, pred)) <= tol
    assert np.abs(np.array(ref["per_class"]) - sk.f1_score(labels, pred, average=None, zero_division=0)).max() <= tol
    assert abs(Fraction(ref["macro"]) - ref["macro_exact"]) <= Fraction(1, 2 ** 52)


def test_threshold_is_strict_and_in_float32():
    scores = np.array([[np.float32(0.2), np.nextafter(np.float32(0.2), np.float32(1)), -0.0, 0.0]], np.float32)
    labels = np.ones((1, 4), np.float32)
    assert float(np.float32(0.2)) > 0.2                # in fp64 it would count
    assert threshold_counts_ref(labels, scores, 0.2)[:, 0].tolist() == [0, 1, 0, 0]
    assert threshold_counts_ref(labels, scores, 0.0)[:, 0].tolist() == [1, 1, 0, 0]
    assert threshold_counts_ref(labels, scores, 0.2)[:, 2].tolist() == [1, 0, 1, 1]


def test_hand_computed_values():
    # descending: 0.9 (+), 0.5 (-, +: one group), 0.1 (-): P = N = 2, two_u = 1 * (1 + 2) + 1 * (2 + 2) = 7
    assert roc_auc_column([1, 0, 1, 0], [0.9, 0.5, 0.5, 0.1]) == (7, 2, 2, 3)
    ref = roc_auc_ref(*make_case("3x2_signed_zeros"))
    # column 0: {-0.0, +0.0} one group with a positive and a negative, then the positive at -1.0: 1 * (0 + 1) / (2 * 2)
    assert ref["two_u"] == [1, 2] and ref["auc"].tolist() == [0.25, 0.5] and ref["groups"].tolist() == [2, 1]
    ref = roc_auc_ref(*make_case("131072x1"))
    assert ref["two_u"][0] > 2 ** 32 and ref["groups"][0] == 16


# ---- the kernel's scheme in numpy, with tiles of 8 positions --------------------------------------------------------
TILE = 8


def _tile_model(y, s):
    """two_u, P the way ap_tile_kernel / auc_terms_kernel get them: records per tile, then per tile the groups that END
    in it, the group that straddles the tile's start seeded by walking the earlier tiles' tail records backwards."""
    s = np.asarray(s).astype(np.float64) + 0.0         # -0.0 -> +0.0
    order = np.argsort(-s, kind="stable")
    s, y = s[order], np.asarray(y).astype(np.int64)[order]
    n = len(s)
    start = np.r_[True, s[1:] != s[:-1]]
    nt = (n + TILE - 1) // TILE
    recs = []
    for b in range(nt):
        lo, hi = b * TILE, min(n, (b + 1) * TILE)
        began = start[lo:hi].nonzero()[0]
        tail0 = lo + began[-1] if len(began) else lo
        recs.append((int(y[lo:hi].sum()), int(y[tail0:hi].sum()), len(began) > 0, hi - tail0))
    two_u = 0
    for b in range(nt):
        lo, hi = b * TILE, min(n, (b + 1) * TILE)
        tp = sum(r[0] for r in recs[:b])
        grp = length = 0
        if b > 0 and not start[lo]:
            for i in range(b - 1, -1, -1):
                grp += recs[i][1]
                length += recs[i][3]
                if recs[i][2]:
                    break
        for p in range(lo, hi):
            if start[p]:
                grp = length = 0
            grp += int(y[p])
            length += 1
            tp += int(y[p])
            if p == n - 1 or start[p + 1]:
                two_u += (length - grp) * (2 * tp - grp)
    return two_u, sum(r[0] for r in recs)


def test_tile_model_matches_the_yardstick():
    rng = np.random.default_rng(77)
    for trial in range(300):
        n = int(rng.integers(1, 70))
        kind = trial % 4
        s = rng.random(n).astype(np.float32)
        if kind == 1:
            s = (np.round(s * 4) / 4).astype(np.float32)          # tie groups across several tiles
        elif kind == 2:
            s = rng.choice(np.array([-0.0, 0.0, 0.5], np.float32), n)
        elif kind == 3:
            s = np.full(n, 0.25, np.float32)
        y = (rng.random(n) < rng.choice([0.1, 0.5, 0.9])).astype(np.float32)
        two_u, P, _, _ = roc_auc_column(y, s)
        assert _tile_model(y, s) == (two_u, P), (trial, n)


# ---- exports ---------------------------------------------------------------------------------------------------------
def test_library_exports_ranking_metrics():
    import ctypes

    from audio_tokens_amd import _lib
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("at_ranking_metrics_f32", "at_threshold_counts_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert getattr(_lib.load(), name) is not None


def test_ops_and_calculator_are_importable():
    from audio_tokens_amd import ops
    from audio_tokens_amd.utils import MetricsCalculator
    for name in ("roc_auc", "mean_roc_auc", "roc_auc_score", "d_prime", "f1_score", "hamming_loss", "classification_metrics"):
        assert callable(getattr(ops, name)) and name in ops.__all__
    assert callable(MetricsCalculator.compute_all_metrics) and callable(MetricsCalculator().compute_metrics)


def test_d_prime_on_the_host():
    from statistics import NormalDist

    from audio_tokens_amd.ops import d_prime
    assert d_prime(0.5) == 0.0
    assert d_prime(0.9) == math.sqrt(2.0) * NormalDist().inv_cdf(0.9)
    assert d_prime(1.0) == math.inf and d_prime(0.0) == -math.inf and math.isnan(d_prime(float("nan")))


def test_f1_and_hamming_from_counts():
    from audio_tokens_amd.ops import _f1_and_hamming
    counts = [[3, 1, 2], [0, 0, 0], [0, 4, 0], [5, 0, 0]]
    per_class, micro, macro, hamming = _f1_and_hamming(counts, 10)
    ref = f1_hamming_ref(np.array(counts), 10)
    assert per_class == ref["per_class"] == [6 / 9, 0.0, 0.0, 1.0]
    assert (micro, macro, hamming) == (ref["micro"], ref["macro"], ref["hamming"]) == (16 / 23, math.fsum(per_class) / 4, 7 / 40)
    assert _f1_and_hamming([[0, 0, 0]], 5)[1:] == (0.0, 0.0, 0.0)
