"""at_average_precision_f32 / ops.average_precision / MetricsCalculator on the MI355X against the exact yardstick
(tests/average_precision_ref.py) and, where it imports, sklearn.

Bounds: per class 2 (P + 2) 2^-53 against the yardstick and 8 (P + 1) 2^-53 against sklearn, P the
class's positives; for the mAP the mean of the per-class bounds plus 2^-52, held in exact rational arithmetic against
the exact mean of the yardstick's values."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from average_precision_ref import ap_bound, average_precision_ref, map_bound_exact, mean_exact, sklearn_bound

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234663852886e38)


def _labels(rng, n, c, per_row=2.0):
    return (rng.random((n, c)) < min(0.5, per_row / c)).astype(np.float32)


def _make(name):
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
    raise KeyError(name)


CASES = ["1x1", "2x1_tied", "3x2_signed_zeros", "63x1", "64x5", "65x7", "257x543", "2216x543_sigmoid",
         "70001x3_continuous", "70001x3_all_equal", "70001x3_saturated", "300x4_extremes", "500x6_degenerate"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(labels, scores, yardstick) of a case, made once and shared (read only)."""
    labels, scores = _make(name)
    ref = average_precision_ref(labels, scores)
    for a in (labels, scores, ref[0], ref[1]):
        a.setflags(write=False)
    return labels, scores, ref


def _run(be, labels, scores):
    ap, n_pos, pair = be.average_precision(scores, labels)
    flags = int(be.ap_flags.item())
    return be.to_host(ap), be.to_host(n_pos), be.to_host(pair), flags


def _hold_to_yardstick(ap, n_pos, pair, ref, what):
    ref_ap, ref_pos, ref_map = ref
    assert np.array_equal(n_pos, ref_pos), what
    assert np.array_equal(np.isnan(ap), ref_pos == 0), what
    live = ref_pos > 0
    bounds = ap_bound(ref_pos)
    err = np.abs(ap[live] - ref_ap[live])
    print(f"{what}: max |ap - ref| = {err.max() if err.size else 0.0:.3e} "
          f"({(err / bounds[live]).max() if err.size else 0.0:.3f} of the bound)")
    assert (err <= bounds[live]).all(), (what, err.max())
    assert pair[1] == live.sum(), what
    got = Fraction(float(pair[0])) / Fraction(int(pair[1])) if pair[1] > 0 else Fraction(0)
    m = float(pair[0]) / float(pair[1]) if pair[1] > 0 else 0.0
    exact = mean_exact(ref_ap, ref_pos)
    mb = map_bound_exact(bounds, ref_pos)
    print(f"{what}: mAP {m!r} vs {ref_map!r}")
    assert abs(Fraction(m) - exact) <= mb, (what, m, ref_map)
    assert abs(got - exact) <= mb, what


@pytest.mark.parametrize("name", CASES)
def test_matches_the_yardstick(be, name):
    labels, scores, ref = _case(name)
    ap, n_pos, pair, flags = _run(be, labels, scores)
    assert flags == 0
    _hold_to_yardstick(ap, n_pos, pair, ref, name)


def test_all_equal_scores_give_the_prevalence(be):
    labels, scores, _ = _case("70001x3_all_equal")
    ap, n_pos, _, _ = _run(be, labels, scores)
    n = labels.shape[0]
    for j in range(3):
        exact = Fraction(int(n_pos[j]), n)
        assert abs(Fraction(float(ap[j])) - exact) <= Fraction(float(ap_bound(n_pos)[j])), j


def test_signed_zeros_value(be):
    labels, scores, _ = _case("3x2_signed_zeros")
    ap, n_pos, _, _ = _run(be, labels, scores)
    # column 0: {-0.0, +0.0} is one group with one positive of two, then -1.0: 1/2 * 1/2 + 1/2 * 2/3
    assert n_pos.tolist() == [2, 2]
    assert abs(ap[0] - (0.25 + 1.0 / 3.0)) <= ap_bound(2)
    # column 1: all three scores are one group: P / N
    assert abs(ap[1] - 2.0 / 3.0) <= ap_bound(2)


def test_matches_sklearn_loop(be):
    sk = pytest.importorskip("sklearn.metrics")
    labels, scores, _ = _case("2216x543_sigmoid")
    ap, n_pos, pair, _ = _run(be, labels, scores)
    bounds = sklearn_bound(n_pos)
    theirs = []
    for j in range(labels.shape[1]):
        if labels[:, j].sum() > 0:
            t = sk.average_precision_score(labels[:, j], scores[:, j])
            assert abs(ap[j] - t) <= bounds[j], (j, ap[j], t)
            theirs.append(t)
    from audio_tokens_amd.ops import mean_average_precision
    m = mean_average_precision(labels, scores, backend=be)
    assert m == float(pair[0]) / float(pair[1])
    # np.mean: at most len(theirs) roundings of a sum <= len(theirs), then one division
    slack = Fraction(len(theirs) + 1, 2 ** 53)
    assert abs(Fraction(m) - Fraction(float(np.mean(theirs)))) <= map_bound_exact(bounds, n_pos) + slack


def _bits(be, labels, scores):
    ap, n_pos, pair = be.average_precision(scores, labels)
    return (be.to_host(ap).view(np.uint64).copy(), be.to_host(n_pos).copy(), be.to_host(pair).view(np.uint64).copy())


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["2216x543_sigmoid", "70001x3_saturated"])
def test_two_calls_give_the_same_bits(be, name):
    labels, scores, _ = _case(name)
    y, s = be.from_host(labels), be.from_host(scores)
    assert _same(_bits(be, y, s), _bits(be, y, s))


def test_chunking_leaves_the_bits_alone(be):
    labels, scores, ref = _case("257x543")
    y, s = be.from_host(labels), be.from_host(scores)
    default = be.debug_get("ap_ws_mb")
    assert default == 1024
    try:
        whole = _bits(be, y, s)                       # 1 GiB: all 543 classes in one chunk
        got = {}
        for setting in (-1, -7, -543, 1):             # chunks of 1, 7, 543 classes; 1 MiB = 255 classes
            be.debug_set("ap_ws_mb", setting)
            got[setting] = _bits(be, y, s)
    finally:
        be.debug_set("ap_ws_mb", default)
    for setting, bits in got.items():
        assert _same(whole, bits), setting
    _hold_to_yardstick(whole[0].view(np.float64), whole[1], whole[2].view(np.float64), ref, "257x543 in chunks")


def test_strided_views_and_other_dtypes(be):
    from audio_tokens_amd.ops import average_precision, mean_average_precision
    rng = np.random.default_rng(11)
    n, wide = 301, 256
    scores16 = torch.from_numpy(rng.random((n, wide)).astype(np.float16)).to(be.device)
    labels_b = torch.from_numpy(rng.random((n, wide)) < 0.1).to(be.device)
    s32, y32 = scores16.float(), labels_b.float()
    want = _bits(be, y32[:, 10:200].contiguous(), s32[:, 10:200].contiguous())
    # a column slice of the wider tensors: passed by its row stride
    view_s, view_y = s32[:, 10:200], y32[:, 10:200]
    assert not view_s.is_contiguous() and be._f32_rows(view_s).data_ptr() == view_s.data_ptr()
    assert _same(want, _bits(be, view_y, view_s))
    # fp16 scores and bool / integer labels through ops, on the device and on the host
    want_ap = want[0].view(np.float64)
    for y, s in ((labels_b[:, 10:200], scores16[:, 10:200]),
                 (labels_b[:, 10:200].to(torch.int32), scores16[:, 10:200]),
                 (labels_b[:, 10:200].cpu().numpy(), scores16[:, 10:200].cpu().numpy())):
        got = average_precision(y, s, backend=be)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want[0])
    pair = want[2].view(np.float64)
    assert mean_average_precision(view_y, view_s, backend=be) == pair[0] / pair[1]
    assert np.isnan(want_ap).sum() == (want[1] == 0).sum()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_scores_raise(be, bad):
    from audio_tokens_amd.ops import average_precision, mean_average_precision
    labels, scores, _ = _case("65x7")
    s = scores.copy()
    s[41, 3] = bad
    with pytest.raises(ValueError, match="NaN or infinity"):
        average_precision(labels, s, backend=be)
    with pytest.raises(ValueError, match="NaN or infinity"):
        mean_average_precision(labels, s, backend=be)


@pytest.mark.parametrize("bad", [0.5, 2.0])
def test_labels_other_than_0_and_1_raise(be, bad):
    from audio_tokens_amd.ops import mean_average_precision
    labels, scores, _ = _case("65x7")
    y = labels.copy()
    y[64, 6] = bad
    with pytest.raises(ValueError, match="0 or 1"):
        mean_average_precision(y, scores, backend=be)
    # and the flag word clears again with the next call
    assert mean_average_precision(labels, scores, backend=be) > 0.0


@pytest.mark.parametrize("shape", [(0, 4), (4, 0)])
def test_empty_input_is_rejected_before_any_launch(be, shape):
    from audio_tokens_amd._lib import NativeError
    z = torch.zeros(shape, dtype=torch.float32, device=be.device)
    with pytest.raises(NativeError, match="at_average_precision_f32: bad sizes"):
        be.average_precision(z, z)


def test_metrics_calculator(be):
    from audio_tokens_amd.utils import MetricsCalculator
    rng = np.random.default_rng(5)
    c = 20
    preds = [rng.random((b, c)).astype(np.float32) for b in (16, 16, 5)]
    labs = [(rng.random((b, c)) < 0.15).astype(np.float32) for b in (16, 16, 5)]
    on_host = MetricsCalculator().compute_metrics(preds, labs)
    on_device = MetricsCalculator.compute_metrics([be.from_host(p) for p in preds], [be.from_host(y) for y in labs])
    assert set(on_host) == {"mAP"} and isinstance(on_host["mAP"], float)
    assert on_host["mAP"] == on_device["mAP"]
    ref_ap, ref_pos, _ = average_precision_ref(np.concatenate(labs), np.concatenate(preds))
    assert abs(Fraction(on_host["mAP"]) - mean_exact(ref_ap, ref_pos)) <= map_bound_exact(ap_bound(ref_pos), ref_pos)
    zeros = np.zeros((37, c), np.float32)
    assert MetricsCalculator.calculate_mAP(zeros, np.concatenate(preds)) == 0.0
    assert MetricsCalculator.calculate_mAP(be.from_host(zeros), be.from_host(np.concatenate(preds))) == 0.0
