"""CPU checks of the average-precision yardstick (tests/average_precision_ref.py) against sklearn, and of the library's
export."""
from fractions import Fraction

import numpy as np
import pytest

from average_precision_ref import average_precision_ref, map_bound_exact, sklearn_bound


def _sklearn_map(labels, scores):
    """What the reference's MetricsCalculator.calculate_mAP computes: sklearn per class with a positive, np.mean."""
    from sklearn.metrics import average_precision_score
    aps = [average_precision_score(labels[:, j], scores[:, j]) for j in range(labels.shape[1]) if labels[:, j].sum() > 0]
    return (float(np.mean(aps)) if aps else 0.0), aps


def _case(n, quantised, seed):
    rng = np.random.default_rng(seed)
    c = 6
    scores = rng.random((n, c)).astype(np.float32)
    if quantised:
        scores = (np.round(scores * 8) / 8).astype(np.float32)
    labels = (rng.random((n, c)) < 0.3).astype(np.float32)
    labels[:, 0] = 1.0                       # an all-positive column
    labels[:, 1] = 0.0                       # a column without positives: skipped
    labels[rng.integers(n), 2] = 1.0         # at least one positive here
    return labels, scores


def _check(labels, scores):
    sk = pytest.importorskip("sklearn.metrics")
    ap, n_pos, m = average_precision_ref(labels, scores)
    assert np.array_equal(n_pos, labels.sum(0).astype(np.int64))
    assert np.array_equal(np.isnan(ap), n_pos == 0)
    bounds = sklearn_bound(n_pos)
    for j in range(labels.shape[1]):
        if n_pos[j] > 0:
            theirs = sk.average_precision_score(labels[:, j], scores[:, j])
            assert abs(ap[j] - theirs) <= bounds[j], (j, ap[j], theirs, n_pos[j])
    ref_mean, aps = _sklearn_map(labels, scores)
    # np.mean adds at most len(aps) roundings of a sum <= len(aps), then one division
    slack = Fraction(len(aps) + 1, 2 ** 53)
    assert abs(Fraction(m) - Fraction(ref_mean)) <= map_bound_exact(bounds, n_pos) + slack


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 65, 2216])
def test_yardstick_matches_sklearn(n, quantised):
    _check(*_case(n, quantised, 100 + n))


def test_signed_zeros_are_one_group():
    scores = np.array([[-0.0], [0.0], [0.5], [-0.25]], np.float32)
    labels = np.array([[1.0], [0.0], [0.0], [1.0]], np.float32)
    _check(labels, scores)
    ap, n_pos, _ = average_precision_ref(labels, scores)
    # groups: 0.5 (no positive), {-0.0, +0.0} (one positive of two), -0.25: 1/2 * 1/3 + 1/2 * 2/4
    assert n_pos[0] == 2 and ap[0] == pytest.approx(1 / 6 + 1 / 4, abs=2 ** -52)


def test_no_positive_anywhere_is_zero():
    pytest.importorskip("sklearn.metrics")
    scores = np.random.default_rng(3).random((17, 4)).astype(np.float32)
    labels = np.zeros((17, 4), np.float32)
    ap, n_pos, m = average_precision_ref(labels, scores)
    assert np.isnan(ap).all() and (n_pos == 0).all() and m == 0.0
    assert _sklearn_map(labels, scores)[0] == 0.0


def test_library_exports_average_precision():
    import ctypes

    from audio_tokens_amd import _lib
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(lib, "at_average_precision_f32")
    assert "at_average_precision_f32" in _lib.SIGNATURES
    assert _lib.load().at_average_precision_f32 is not None


def test_metrics_calculator_is_importable():
    from audio_tokens_amd.ops import average_precision, mean_average_precision  # noqa: F401
    from audio_tokens_amd.utils import MetricsCalculator
    from audio_tokens_amd.utils.metrics_calculator import MetricsCalculator as M2
    assert MetricsCalculator is M2
    assert callable(MetricsCalculator.compute_metrics) and callable(MetricsCalculator().calculate_mAP)
