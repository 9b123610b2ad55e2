"""at_ranking_metrics_f32 / at_threshold_counts_f32, ops.roc_auc ... classification_metrics and
MetricsCalculator.compute_all_metrics on the MI355X against the exact yardstick (tests/roc_auc_ref.py).

two_u, n_pos and the threshold counts are integers and auc, F1 (micro, per class) and the Hamming loss one correctly
rounded division of them: all are held bit for bit.  mauc[0] / mauc[1] is held within 2^-52 of the exact mean of the auc
values in rational arithmetic, and the average precision of the combined call to at_average_precision_f32's bits."""
import functools
import math
from fractions import Fraction
from statistics import NormalDist

import numpy as np
import pytest
import torch

from roc_auc_ref import CASES, f1_hamming_ref, make_case, mean_exact, roc_auc_ref, threshold_counts_ref

pytestmark = pytest.mark.gpu

KEYS = ("auc", "two_u", "n_pos", "mauc", "ap", "map")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(labels, scores, yardstick) of a case, made once and shared (read only)."""
    labels, scores = make_case(name)
    ref = roc_auc_ref(labels, scores)
    for a in (labels, scores, ref["auc"], ref["n_pos"]):
        a.setflags(write=False)
    return labels, scores, ref


def _bits(be, labels, scores, want_ap=True):
    """The call's outputs on the host, doubles as their bit patterns (NaN compares equal to itself that way)."""
    out = be.ranking_metrics(scores, labels, want_ap=want_ap)
    assert int(be.ap_flags.item()) == 0
    host = {}
    for k in KEYS:
        if out[k] is not None:
            a = be.to_host(out[k])
            host[k] = a.view(np.uint64).copy() if a.dtype == np.float64 else a.copy()
    return host


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def _hold_to_yardstick(got, ref, what):
    assert got["two_u"].tolist() == ref["two_u"], what
    assert np.array_equal(got["n_pos"], ref["n_pos"]), what
    assert np.array_equal(got["auc"], ref["auc"].view(np.uint64)), what       # NaN where P or N is 0 included
    defined = ~np.isnan(ref["auc"])
    total, count = got["mauc"].view(np.float64)
    assert count == defined.sum(), what
    if count > 0:
        m = float(total) / float(count)
        print(f"{what}: mAUC {m!r} vs {float(ref['mean'])!r}")
        assert abs(Fraction(m) - ref["mean"]) <= Fraction(1, 2 ** 52), what
    else:
        assert total == 0.0, what


@pytest.mark.parametrize("name", CASES)
def test_matches_the_yardstick_and_average_precision(be, name):
    labels, scores, ref = _case(name)
    y, s = be.from_host(labels), be.from_host(scores)
    got = _bits(be, y, s)
    _hold_to_yardstick(got, ref, name)
    ap, n_pos, pair = be.average_precision(s, y)
    assert np.array_equal(got["ap"], be.to_host(ap).view(np.uint64)), name
    assert np.array_equal(got["n_pos"], be.to_host(n_pos)), name
    assert np.array_equal(got["map"], be.to_host(pair).view(np.uint64)), name


def test_wide_accumulators(be):
    labels, scores, ref = _case("131072x1")
    assert ref["two_u"][0] > 2 ** 32
    assert _bits(be, labels, scores, want_ap=False)["two_u"].tolist() == ref["two_u"]


def test_chunking_leaves_the_bits_alone(be):
    labels, scores, ref = _case("257x543")
    y, s = be.from_host(labels), be.from_host(scores)
    default = be.debug_get("ap_ws_mb")
    try:
        whole = _bits(be, y, s)                       # all 543 classes in one chunk
        got = {}
        for setting in (-1, -7, -543):                # chunks of 1, 7, 543 classes
            be.debug_set("ap_ws_mb", setting)
            got[setting] = _bits(be, y, s)
    finally:
        be.debug_set("ap_ws_mb", default)
    for setting, bits in got.items():
        assert _same(whole, bits), setting
    _hold_to_yardstick(whole, ref, "257x543 in chunks")


@pytest.mark.parametrize("name", ["2216x543_sigmoid", "70001x3_saturated"])
def test_two_calls_give_the_same_bits(be, name):
    labels, scores, _ = _case(name)
    y, s = be.from_host(labels), be.from_host(scores)
    assert _same(_bits(be, y, s), _bits(be, y, s))


def test_strided_views_other_dtypes_and_no_ap(be):
    from audio_tokens_amd.ops import mean_roc_auc, roc_auc, roc_auc_score
    rng = np.random.default_rng(11)
    n, wide = 301, 256
    scores16 = torch.from_numpy(rng.random((n, wide)).astype(np.float16)).to(be.device)
    labels_b = torch.from_numpy(rng.random((n, wide)) < 0.1).to(be.device)
    s32, y32 = scores16.float(), labels_b.float()
    want = _bits(be, y32[:, 10:200].contiguous(), s32[:, 10:200].contiguous())
    ref = roc_auc_ref(y32[:, 10:200].cpu().numpy(), s32[:, 10:200].cpu().numpy())
    _hold_to_yardstick(want, ref, "301x190")
    # a column slice of the wider tensors: passed by its row stride
    view_s, view_y = s32[:, 10:200], y32[:, 10:200]
    assert not view_s.is_contiguous() and be._f32_rows(view_s).data_ptr() == view_s.data_ptr()
    assert _same(want, _bits(be, view_y, view_s))
    # without the average precision: the same ROC AUC, and no ap / map
    bare = _bits(be, view_y, view_s, want_ap=False)
    assert set(bare) == {"auc", "two_u", "n_pos", "mauc"} and all(np.array_equal(bare[k], want[k]) for k in bare)
    # fp16 scores and bool / integer labels through ops, on the device and on the host
    for y, s in ((labels_b[:, 10:200], scores16[:, 10:200]),
                 (labels_b[:, 10:200].to(torch.int32), scores16[:, 10:200]),
                 (labels_b[:, 10:200].cpu().numpy(), scores16[:, 10:200].cpu().numpy())):
        got = roc_auc(y, s, backend=be)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want["auc"])
    total, count = want["mauc"].view(np.float64)
    assert mean_roc_auc(view_y, view_s, backend=be) == total / count
    # one column through the 1-D entry
    j = int(np.flatnonzero(~np.isnan(ref["auc"]))[0])
    assert roc_auc_score(labels_b[:, 10 + j], scores16[:, 10 + j], backend=be) == ref["auc"][j]
    assert roc_auc_score(view_y[:, j].cpu().numpy(), view_s[:, j].cpu().numpy(), backend=be) == ref["auc"][j]


def test_one_class_only_raises_sklearns_error(be):
    from audio_tokens_amd.ops import mean_roc_auc, roc_auc, roc_auc_score
    s = np.linspace(0, 1, 9, dtype=np.float32)
    for y in (np.zeros(9, np.float32), np.ones(9, np.float32)):
        with pytest.raises(ValueError, match="Only one class present in y_true. ROC AUC score is not defined in that case."):
            roc_auc_score(y, s, backend=be)
        assert np.isnan(roc_auc(y[:, None], s[:, None], backend=be)).all()
        assert mean_roc_auc(y[:, None], s[:, None], backend=be) == 0.0


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_scores_raise(be, bad):
    from audio_tokens_amd import ops
    labels, scores, _ = _case("65x7")
    s = scores.copy()
    s[41, 3] = bad
    be.ranking_metrics(s, labels)
    assert int(be.ap_flags.item()) == 1
    be.threshold_counts(s, labels, 0.2)
    assert int(be.tc_flags.item()) == 1
    for call in (lambda: ops.roc_auc(labels, s, backend=be), lambda: ops.mean_roc_auc(labels, s, backend=be),
                 lambda: ops.f1_score(labels, s, 0.2, backend=be), lambda: ops.hamming_loss(labels, s, 0.2, backend=be),
                 lambda: ops.classification_metrics(labels, s, backend=be)):
        with pytest.raises(ValueError, match="NaN or infinity"):
            call()


@pytest.mark.parametrize("bad", [0.5, 2.0])
def test_labels_other_than_0_and_1_raise(be, bad):
    from audio_tokens_amd import ops
    labels, scores, _ = _case("65x7")
    y = labels.copy()
    y[64, 6] = bad
    be.ranking_metrics(scores, y)
    assert int(be.ap_flags.item()) == 2
    be.threshold_counts(scores, y, 0.2)
    assert int(be.tc_flags.item()) == 2
    for call in (lambda: ops.mean_roc_auc(y, scores, backend=be), lambda: ops.f1_score(y, scores, 0.2, backend=be),
                 lambda: ops.classification_metrics(y, scores, backend=be)):
        with pytest.raises(ValueError, match="0 or 1"):
            call()
    # and the flag words clear again with the next call
    assert ops.mean_roc_auc(labels, scores, backend=be) > 0.0
    assert ops.hamming_loss(labels, scores, 0.2, backend=be) > 0.0


def test_on_a_second_stream(be):
    labels, scores, _ = _case("65x7")
    y, s = be.from_host(labels), be.from_host(scores)
    want = _bits(be, y, s)
    want_counts = be.to_host(be.threshold_counts(s, y, 0.2))
    side = torch.cuda.Stream(device=be.device)
    side.wait_stream(torch.cuda.current_stream(be.device))
    with torch.cuda.stream(side):
        got = _bits(be, y, s)
        got_counts = be.to_host(be.threshold_counts(s, y, 0.2))
    side.synchronize()
    assert _same(want, got) and np.array_equal(want_counts, got_counts)
    assert _same(want, _bits(be, y, s))               # and back on the first one


@pytest.mark.parametrize("shape", [(0, 4), (4, 0)])
def test_empty_input_is_rejected_before_any_launch(be, shape):
    from audio_tokens_amd._lib import NativeError
    z = torch.zeros(shape, dtype=torch.float32, device=be.device)
    with pytest.raises(NativeError, match="at_ranking_metrics_f32: bad sizes"):
        be.ranking_metrics(z, z)
    with pytest.raises(NativeError, match="at_threshold_counts_f32: bad sizes"):
        be.threshold_counts(z, z, 0.2)


# ---- threshold counts ---------------------------------------------------------------------------------------------
def _threshold_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    n, c = map(int, name.split("x"))
    scores = rng.random((n, c)).astype(np.float32)
    scores[rng.random((n, c)) < 0.2] = np.float32(0.2)           # exactly the threshold in fp32: not predicted
    scores[rng.random((n, c)) < 0.1] = np.float32(-0.0)
    scores[rng.random((n, c)) < 0.1] = np.float32(0.0)
    labels = (rng.random((n, c)) < 0.3).astype(np.float32)
    if c > 2:
        labels[:, 1] = 0.0                                       # a class with no positives and no predictions
        scores[:, 1] = 0.1
    return labels, scores


@pytest.mark.parametrize("name", ["1x1", "1x65", "37x1", "300x64", "300x65", "301x543", "3x5000"])
@pytest.mark.parametrize("threshold", [0.2, 0.0])
def test_threshold_counts_equal_numpys(be, name, threshold):
    from audio_tokens_amd.ops import f1_score, hamming_loss
    labels, scores = _threshold_case(name)
    n, c = labels.shape
    want = threshold_counts_ref(labels, scores, threshold)
    pred = scores > threshold                                    # numpy: float32 against a Python float
    assert np.array_equal(want[:, 0] + want[:, 1], pred.sum(0))
    if threshold == 0.2:
        assert not pred[scores == np.float32(0.2)].any() and float(np.float32(0.2)) > 0.2
    else:
        assert not pred[scores == 0.0].any() and (n * c < 300 or (np.signbit(scores) & (scores == 0.0)).any())
    y, s = be.from_host(labels), be.from_host(scores)
    got = be.to_host(be.threshold_counts(s, y, threshold))
    assert int(be.tc_flags.item()) == 0
    assert got.dtype == np.int64 and np.array_equal(got, want), name
    if c > 2 and threshold == 0.2:
        assert want[1].tolist() == [0, 0, 0]
    ref = f1_hamming_ref(want, n)
    assert f1_score(y, s, threshold, average="micro", backend=be) == ref["micro"]
    assert f1_score(y, s, threshold, average="macro", backend=be) == ref["macro"]
    assert f1_score(y, s, threshold, average=None, backend=be).tolist() == ref["per_class"]
    assert hamming_loss(y, s, threshold, backend=be) == ref["hamming"]
    assert abs(Fraction(ref["macro"]) - ref["macro_exact"]) <= Fraction(1, 2 ** 52)


def test_threshold_counts_on_a_strided_view(be):
    labels, scores = _threshold_case("301x543")
    y, s = be.from_host(labels), be.from_host(scores)
    view_y, view_s = y[:, 100:443], s[:, 100:443]
    assert not view_s.is_contiguous()
    got = be.to_host(be.threshold_counts(view_s, view_y, 0.2))
    assert np.array_equal(got, threshold_counts_ref(labels[:, 100:443], scores[:, 100:443], 0.2))


def test_threshold_metrics_match_sklearn(be):
    sk = pytest.importorskip("sklearn.metrics")
    from audio_tokens_amd.ops import f1_score, hamming_loss
    labels, scores = _threshold_case("301x543")
    pred = scores > 0.2
    tol = 2.0 ** -52
    assert abs(f1_score(labels, scores, 0.2, average="micro", backend=be)
               - sk.f1_score(labels, pred, average="micro", zero_division=0)) <= tol
    assert abs(f1_score(labels, scores, 0.2, average="macro", backend=be)
               - sk.f1_score(labels, pred, average="macro", zero_division=0)) <= tol
    assert abs(hamming_loss(labels, scores, 0.2, backend=be) - sk.hamming_loss(labels, pred)) <= tol


# ---- the whole dict -----------------------------------------------------------------------------------------------
def test_metrics_calculator_compute_all_metrics(be):
    from audio_tokens_amd.ops import classification_metrics
    from audio_tokens_amd.utils import MetricsCalculator
    rng = np.random.default_rng(5)
    c = 20
    preds = [rng.random((b, c)).astype(np.float32) for b in (16, 16, 5)]          # a short last batch
    labs = [(rng.random((b, c)) < 0.15).astype(np.float32) for b in (16, 16, 5)]
    on_host = MetricsCalculator().compute_all_metrics(preds, labs)
    on_device = MetricsCalculator.compute_all_metrics([be.from_host(p) for p in preds], [be.from_host(y) for y in labs])
    assert set(on_host) == {"mAP", "mAUC", "d_prime", "f1_score_micro", "f1_score_macro", "hamming_loss"}
    assert all(isinstance(v, float) for v in on_host.values())
    assert on_host == on_device
    assert on_host["d_prime"] == math.sqrt(2.0) * NormalDist().inv_cdf(on_host["mAUC"])
    assert MetricsCalculator.compute_metrics(preds, labs) == {"mAP": on_host["mAP"]}
    all_y, all_p = np.concatenate(labs), np.concatenate(preds)
    ref = roc_auc_ref(all_y, all_p)
    assert abs(Fraction(on_host["mAUC"]) - mean_exact(ref["auc"], ~np.isnan(ref["auc"]))) <= Fraction(1, 2 ** 52)
    f1 = f1_hamming_ref(threshold_counts_ref(all_y, all_p, 0.2), len(all_y))
    assert (on_host["f1_score_micro"], on_host["f1_score_macro"], on_host["hamming_loss"]) == \
        (f1["micro"], f1["macro"], f1["hamming"])
    other = MetricsCalculator.compute_all_metrics(preds, labs, prediction_threshold=0.5)
    f5 = f1_hamming_ref(threshold_counts_ref(all_y, all_p, 0.5), len(all_y))
    assert other["hamming_loss"] == f5["hamming"] and other["mAUC"] == on_host["mAUC"]
    assert classification_metrics(all_y, all_p, backend=be) == on_host
