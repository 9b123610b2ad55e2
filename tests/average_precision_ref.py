"""The yardstick of at_average_precision_f32: sklearn's average_precision_score per class as a closed form over the
groups of equal scores, with exact integer counts and a correctly rounded sum.

For one column, sorted by score descending and cut into groups of equal scores (-0.0 == +0.0):
    AP = sum_g (tp_g - tp_{g-1}) / P * tp_g / cnt_g
tp_g, cnt_g = positives / samples seen up to the end of group g, P = all positives.  Each term is computed in fp64
(three roundings), the terms are added with math.fsum (one rounding).  Classes without a positive give NaN and are left
out of the mean; the mean of no class is 0.0 (the reference's calculate_mAP)."""
import math
from fractions import Fraction

import numpy as np


def average_precision_column(y, s):
    """(AP, P) of one column: y 0/1 [n], s scores [n]."""
    s = np.asarray(s).astype(np.float64)          # exact for float16 / float32 scores
    y = np.asarray(y).astype(np.int64)
    order = np.argsort(-s, kind="stable")
    s, y = s[order], y[order]
    last = np.r_[s[1:] != s[:-1], True]           # the last sample of every group
    tp = np.cumsum(y)[last]
    cnt = np.nonzero(last)[0].astype(np.int64) + 1
    P = int(tp[-1])
    if P == 0:
        return float("nan"), 0
    dtp = np.diff(np.r_[np.int64(0), tp])
    live = dtp > 0                                # the other groups contribute exactly 0
    terms = (dtp[live] / np.int64(P)) * (tp[live] / cnt[live])
    return math.fsum(terms.tolist()), P


def mean_exact(ap, n_pos):
    """The mean of ap over the classes with positives as an exact Fraction (0 when there is none)."""
    live = [Fraction(float(a)) for a, p in zip(ap, n_pos) if p > 0]
    return sum(live, Fraction(0)) / len(live) if live else Fraction(0)


def average_precision_ref(labels, scores):
    """labels, scores [n, c] -> (ap float64 [c] with NaN where a class has no positive, n_pos int64 [c], mAP float:
    the exact mean of the ap values, rounded once)."""
    labels, scores = np.asarray(labels), np.asarray(scores)
    assert labels.shape == scores.shape and labels.ndim == 2
    c = labels.shape[1]
    ap = np.empty(c, np.float64)
    n_pos = np.empty(c, np.int64)
    for j in range(c):
        ap[j], n_pos[j] = average_precision_column(labels[:, j], scores[:, j])
    m = mean_exact(ap, n_pos)
    return ap, n_pos, m.numerator / m.denominator


def ap_bound(n_pos):
    """|ap - yardstick| allowed per class: 2 (P + 2) 2^-53."""
    return 2.0 * (np.asarray(n_pos, np.float64) + 2.0) * 2.0 ** -53


def sklearn_bound(n_pos):
    """against sklearn's own summation: 8 (P + 1) 2^-53."""
    return 8.0 * (np.asarray(n_pos, np.float64) + 1.0) * 2.0 ** -53


def map_bound_exact(bounds, n_pos):
    """The bound on the mAP: the mean of the per-class bounds over the classes with positives, plus 2^-52 (Fraction)."""
    live = [Fraction(float(b)) for b, p in zip(bounds, n_pos) if p > 0]
    return (sum(live, Fraction(0)) / len(live) if live else Fraction(0)) + Fraction(1, 2 ** 52)
