"""The yardstick of at_ranking_metrics_f32's ROC AUC and of at_threshold_counts_f32, in Python integers and Fractions,
and the cases both test files run (tests/test_roc_auc_ref.py on the CPU, tests/test_gpu_ranking_metrics.py on the device).

For one column, sorted by score descending and cut into groups of equal scores (-0.0 == +0.0), with tp_g, fp_g the
positives / negatives up to the end of group g, P and N all of them:
    two_u = sum_g (fp_g - fp_{g-1}) (tp_g + tp_{g-1})        AUC = two_u / (2 P N)
sklearn's roc_auc_score (the trapezoid rule over roc_curve) in exact arithmetic.  auc = float(two_u) / float(2 P N):
Python's int -> float conversion and its division are correctly rounded, as the device's are, so this is the kernel's
expression bit for bit.  Classes without a positive or without a negative give NaN and are left out of the mean.

Threshold metrics: predicted = score > threshold in float32 (numpy's comparison of a float32 array with a Python
float); tp, fp, fn per class; F1 = 2 tp / (2 tp + fp + fn), 0 where that denominator is 0 (sklearn's zero_division=0);
micro from the summed counts; macro over all classes; Hamming loss = (fp + fn) / (n c)."""
import math
from fractions import Fraction

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)


def roc_auc_column(y, s):
    """(two_u, P, N, G) of one column as Python ints: y 0/1 [n], s scores [n]; G = the number of groups."""
    s = np.asarray(s).astype(np.float64)          # exact for float16 / float32 scores
    y = np.asarray(y).astype(np.int64)
    order = np.argsort(-s, kind="stable")
    s, y = s[order], y[order]
    last = np.r_[s[1:] != s[:-1], True]           # the last sample of every group
    tp = np.cumsum(y)[last]
    fp = np.nonzero(last)[0].astype(np.int64) + 1 - tp
    tp0, fp0 = np.r_[np.int64(0), tp[:-1]], np.r_[np.int64(0), fp[:-1]]
    prod = (fp - fp0) * (tp + tp0)                # each <= 2 P N < 2^61: exact in int64
    two_u = sum(int(x) for x in prod[prod != 0])  # added as Python ints
    P = int(tp[-1])
    return two_u, P, len(y) - P, int(last.sum())


def mean_exact(values, defined):
    """The mean of the float values where defined, as an exact Fraction (0 when there is none)."""
    live = [Fraction(float(v)) for v, d in zip(values, defined) if d]
    return sum(live, Fraction(0)) / len(live) if live else Fraction(0)


def roc_auc_ref(labels, scores):
    """labels, scores [n, c] -> dict: two_u (list of Python ints), n_pos, n_neg, groups (int64 [c]), auc (float64 [c],
    NaN where P or N is 0), exact (list of Fraction or None), mean (Fraction: the exact mean of the auc floats)."""
    labels, scores = np.asarray(labels), np.asarray(scores)
    assert labels.shape == scores.shape and labels.ndim == 2
    c = labels.shape[1]
    cols = [roc_auc_column(labels[:, j], scores[:, j]) for j in range(c)]
    auc = np.array([float(u) / float(2 * p * q) if p and q else float("nan") for u, p, q, _ in cols], np.float64)
    return {"two_u": [u for u, _, _, _ in cols], "n_pos": np.array([p for _, p, _, _ in cols], np.int64),
            "n_neg": np.array([q for _, _, q, _ in cols], np.int64), "groups": np.array([g for *_, g in cols], np.int64),
            "auc": auc, "exact": [Fraction(u, 2 * p * q) if p and q else None for u, p, q, _ in cols],
            "mean": mean_exact(auc, ~np.isnan(auc))}


def sklearn_auc_bound(groups):
    """|sklearn's roc_auc_score - the exact AUC| + |auc - the exact AUC| allowed: (G + 10) 2^-53."""
    return (np.asarray(groups, np.float64) + 10.0) * 2.0 ** -53


def threshold_counts_ref(labels, scores, threshold):
    """int64 [c, 3]: tp, fp, fn of scores > threshold, compared in float32 as numpy does."""
    pred = np.asarray(scores).astype(np.float32) > np.float32(threshold)
    true = np.asarray(labels) == 1
    return np.stack([(pred & true).sum(0), (pred & ~true).sum(0), (~pred & true).sum(0)], axis=1).astype(np.int64)


def f1_hamming_ref(counts, n):
    """counts [c, 3] -> dict: per_class (list of floats), micro, macro, hamming (floats: one correctly rounded division of
    exact integers each; macro = fsum(per_class) / c), and macro_exact (Fraction: the mean of the exact ratios)."""
    rows = [tuple(int(v) for v in r) for r in np.asarray(counts)]
    den = [2 * tp + fp + fn for tp, fp, fn in rows]
    per_class = [2 * r[0] / d if d else 0.0 for r, d in zip(rows, den)]
    tp, fp, fn = (sum(col) for col in zip(*rows))
    d = 2 * tp + fp + fn
    return {"per_class": per_class, "micro": 2 * tp / d if d else 0.0, "macro": math.fsum(per_class) / len(rows),
            "hamming": (fp + fn) / (n * len(rows)),
            "macro_exact": sum((Fraction(2 * r[0], d) for r, d in zip(rows, den) if d), Fraction(0)) / len(rows)}


# ---- the cases ---------------------------------------------------------------------------------------------------
def _labels(rng, n, c, per_row=2.0):
    return (rng.random((n, c)) < min(0.5, per_row / c)).astype(np.float32)


def make_case(name):
    """(labels, scores) float32 [n, c]: the constructions of tests/test_gpu_average_precision.py, then two scores with
    the boundary on and beside a tile edge, and a column whose two_u does not fit 32 bits."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "1x1":
        return np.ones((1, 1), np.float32), np.array([[0.3]], np.float32)
    if name == "2x1_tied":
        return np.array([[1.0], [0.0]], np.float32), np.array([[0.7], [0.7]], np.float32)
    if name == "3x2_signed_zeros":
        scores = np.array([[-0.0, 0.0], [0.0, -0.0], [-1.0, 0.0]], np.float32)
        labels = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], np.float32)
        return labels, scores
    if name in ("63x1", "64x5", "65x7", "257x543"):
        n, c = map(int, name.split("x"))
        labels = (rng.random((n, c)) < 0.2).astype(np.float32)
        return labels, rng.random((n, c)).astype(np.float32)
    if name == "2216x543_sigmoid":
        n, c = 2216, 543
        logits = rng.normal(size=(n, c)).astype(np.float32) * 3 - 2
        scores = (1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).astype(np.float32)
        return _labels(rng, n, c), scores
    if name.startswith("70001x3"):
        n, c = 70001, 3
        labels = (rng.random((n, c)) < np.array([0.001, 0.3, 0.9])).astype(np.float32)
        if name.endswith("continuous"):
            scores = rng.random((n, c)).astype(np.float32)
        elif name.endswith("all_equal"):
            scores = np.full((n, c), 0.25, np.float32)
        else:                                        # saturated: exactly 1.0 and 0.0, two huge groups
            scores = (rng.random((n, c)) < 0.4).astype(np.float32)
        return labels, scores
    if name == "300x4_extremes":
        pool = np.array([1e-45, -1e-45, 1e-40, -1e-40, FLT_MAX, -FLT_MAX, 0.0, -0.0, 1.0, 1.1754944e-38, -1.1754944e-38],
                        np.float32)
        scores = pool[rng.integers(0, len(pool), (300, 4))]
        return (rng.random((300, 4)) < 0.3).astype(np.float32), scores
    if name == "500x6_degenerate":
        n, c = 500, 6
        labels = (rng.random((n, c)) < 0.1).astype(np.float32)
        labels[:, 0] = 1.0                           # all positive
        labels[:, 1] = 0.0                           # all negative
        labels[:, 2] = 0.0
        labels[137, 2] = 1.0                         # a single positive
        labels[:, 4] = 0.0
        labels[n - 1, 4] = 1.0
        scores = rng.random((n, c)).astype(np.float32)
        scores[:, 4] = np.round(scores[:, 4] * 4) / 4
        return labels, scores
    if name in ("2047x2", "2048x2", "2049x2", "4097x2"):
        # two distinct scores: column 0's upper group ends on the last tile edge inside the column (or, where there is
        # none, one position before the end), column 1's one position beside that
        n = int(name.split("x")[0])
        edge = (n - 1) // 2048 * 2048 or n - 1
        high = [edge, edge + 1 if edge + 1 < n else edge - 1]
        scores = np.zeros((n, 2), np.float32)
        for j in range(2):
            scores[rng.permutation(n)[:high[j]], j] = 0.75
        return (rng.random((n, 2)) < 0.3).astype(np.float32), scores
    if name == "131072x1":
        # half positives, 16 score levels that lean towards the positives: two_u is well above 2^32
        n = 131072
        labels = np.zeros((n, 1), np.float32)
        labels[rng.permutation(n)[:n // 2], 0] = 1.0
        levels = np.clip(rng.integers(0, 13, (n, 1)) + 3 * labels.astype(np.int64), 0, 15)
        return labels, (levels / 16.0).astype(np.float32)
    raise KeyError(name)


CASES = ["1x1", "2x1_tied", "3x2_signed_zeros", "63x1", "64x5", "65x7", "257x543", "2216x543_sigmoid",
         "70001x3_continuous", "70001x3_all_equal", "70001x3_saturated", "300x4_extremes", "500x6_degenerate",
         "2047x2", "2048x2", "2049x2", "4097x2", "131072x1"]
