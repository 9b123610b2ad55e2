"""The rungs of tests/hard_silhouette_data.py are what their names say, proved with tests/silhouette_ref.py alone (and,
where it imports, with sklearn bit for bit).  tests/test_gpu_hard_silhouette.py compares at_silhouette_f32 with the same
reference bit for bit; without the facts below a rung that silently left the order-free regime, or degenerated into
zeros, would make that comparison wrong or vacuous."""
import functools
import warnings

import numpy as np
import pytest

import hard_silhouette_data as hs
from silhouette_ref import check_labels, silhouette_samples_ref
from test_gpu_silhouette import S_TOL

TINY = np.float32(2.0 ** -126)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _ref(name):
    x, lab = hs.rung(name)
    with np.errstate(all="ignore"):
        s = silhouette_samples_ref(x, lab)
    s.setflags(write=False)
    return s


def _d2(x):
    """fl32(((-2 <x_i, x_j>) + |x_i|^2) + |x_j|^2) of every pair, before the clamp."""
    x64 = x.astype(np.float64)
    nrm = np.einsum("ij,ij->i", x64, x64)
    with np.errstate(all="ignore"):
        return (((-2.0 * (x64 @ x64.T)) + nrm[:, None]) + nrm[None, :]).astype(np.float32)


def _variant(x, labels, descending=False, flush=False):
    """tests/silhouette_ref.py's recipe again, with two switches that a wrong kernel could have: the members of a
    cluster summed in descending j, and a subnormal fp32 d2 flushed to 0."""
    n = x.shape[0]
    enc, k = check_labels(labels, n)
    freq = np.bincount(enc, minlength=k)
    with np.errstate(all="ignore"):
        d2 = np.maximum(_d2(x), np.float32(0))
        if flush:
            d2[d2 < TINY] = 0
        np.fill_diagonal(d2, 0)
        dist = np.sqrt(d2)
        S = np.zeros((n, k), np.float32)
        for r in range(n):
            S[r] = np.bincount(enc[::-1], weights=dist[r, ::-1], minlength=k) if descending else \
                np.bincount(enc, weights=dist[r], minlength=k)
        rows = np.arange(n)
        a = S[rows, enc].copy()
        S[rows, enc] = np.inf
        S /= freq
        b = S.min(axis=1)
        a /= (freq - 1).take(enc)
        return np.nan_to_num((b - a) / np.maximum(a, b))


def _zero_share_outside(name, s):
    """The share of zero scores among the rows that are not planted to score 0."""
    x, lab = hs.rung(name)
    enc, _ = check_labels(lab, len(lab))
    keep = np.bincount(enc)[enc] > 1                                      # not the singletons
    if name == "far":
        keep[hs.facts(name)["displaced"]] = False
    return float((s[keep] == 0).mean()) if keep.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# order-freeness

def test_the_rung_lists():
    assert len(set(hs.ALL)) == len(hs.ALL) and set(hs.GRID) < set(hs.BITWISE)
    assert len(hs.GRID_D) == 18 and len(hs.SEAMS) == 2 * (1 + 10 * 3)
    for name in hs.ALL:
        x, lab = hs.rung(name)
        assert x.dtype == np.float32 and lab.dtype == np.int64 and x.ndim == 2 and lab.shape == (len(x),)
        assert len(x) <= 4500 and np.isfinite(x).all()
        assert hs.rung(name)[0] is x                                      # built once, shared, read-only
        assert not x.flags.writeable and not lab.flags.writeable


@pytest.mark.parametrize("name", hs.GRID)
def test_grid_rungs_meet_the_exactness_bound(name):
    x, _ = hs.rung(name)
    ints = hs.grid_ints(name)
    e = hs.SCALE_EXP.get(name, 0)
    assert np.array_equal(np.ldexp(ints.astype(np.float64), hs.Q_EXP + e), x.astype(np.float64))   # x is on the grid
    assert hs.exactness(ints, x.shape[1]) < 2 ** 53


def test_the_grid_builder_refuses_rows_outside_the_regime():
    with pytest.raises(AssertionError):
        hs.grid(np.full((2, 200), 1 << 22))                               # 4 x 200 x 2^44 > 2^53
    with pytest.raises(AssertionError):
        hs.grid(np.array([[1, 2], [3, 4]]), -130)                         # x leaves the fp32 normal range


@pytest.mark.parametrize("name", hs.BITWISE)
def test_a_permutation_of_the_dimensions_keeps_every_bit(name):
    x, lab = hs.rung(name)
    p = np.random.default_rng(len(name)).permutation(x.shape[1])
    with np.errstate(all="ignore"):
        moved = silhouette_samples_ref(np.ascontiguousarray(x[:, p]), lab)
    assert np.array_equal(bits(moved), bits(_ref(name)))


@pytest.mark.parametrize("name", hs.BITWISE)
def test_sklearn_gives_the_same_bits(name):
    sk = pytest.importorskip("sklearn.metrics")
    x, lab = hs.rung(name)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        theirs = sk.silhouette_samples(x, lab)
    assert theirs.dtype == np.float32
    assert np.array_equal(bits(theirs), bits(_ref(name)))


def test_the_variant_without_switches_is_the_reference():
    for name in ("grid_d-0-65", "order-ones_first", "tiny76", "far", "cancel"):
        x, lab = hs.rung(name)
        assert np.array_equal(bits(_variant(x, lab)), bits(_ref(name))), name


# ---------------------------------------------------------------------------------------------------------------------
# labels, order

def test_label_values_do_not_move_a_bit():
    x, plain = hs.rung("labels-plain")
    assert np.array_equal(np.unique(plain), np.arange(5))
    for name in ("labels-ends", "labels-wide"):
        y, lab = hs.rung(name)
        assert np.array_equal(bits(y), bits(x)) and len(np.unique(lab)) == 5
        assert np.array_equal(bits(_ref(name)), bits(_ref("labels-plain")))
    assert set(hs.rung("labels-ends")[1]) == {hs.I64_MIN, -1, 0, 1, hs.I64_MAX}
    wide = np.unique(hs.rung("labels-wide")[1])
    assert wide[0] < 0 < wide[-1] and np.all(np.diff(wide) >= 2 ** 40)


def test_the_order_of_a_clusters_members_shows_in_row_0():
    first, large, mixed = (_ref("order-" + v) for v in ("ones_first", "large_first", "mixed"))
    print("s[0]: ones first %d, large first %d, mixed %d" % (bits(first)[0], bits(large)[0], bits(mixed)[0]))
    assert bits(first)[0] != bits(large)[0]
    assert bits(first)[0] == 3120549888 and bits(large)[0] == 3120553984
    assert bits(mixed)[0] == bits(first)[0]
    # mixed: the three clusters interleave in row order, and the sorted order is not the row order
    lab = hs.rung("order-mixed")[1]
    assert lab[0] == 0 and np.count_nonzero(np.diff(lab)) >= 4 and np.any(np.diff(lab) < 0)
    for name in hs.ORDER:
        x, lab = hs.rung(name)
        assert x.shape == (2 + hs.N_ONES + 2 + 3, 1) and np.array_equal(np.bincount(lab), [2, hs.N_ONES + 2, 3])
        assert np.all(_ref(name) != 0)


@pytest.mark.parametrize("name", ["order-ones_first", "order-mixed"])
def test_summing_a_cluster_in_descending_order_is_noticed(name):
    x, lab = hs.rung(name)
    wrong = _variant(x, lab, descending=True)
    assert bits(wrong)[0] != bits(_ref(name))[0]
    assert bits(wrong)[0] == bits(_ref("order-large_first"))[0]


# ---------------------------------------------------------------------------------------------------------------------
# magnitude

@pytest.mark.parametrize("name", ["tiny70", "tiny76"])
def test_tiny_lives_in_the_subnormal_range(name):
    x, lab = hs.rung(name)
    d2 = _d2(x)[~np.eye(len(x), dtype=bool)]
    share = float(((d2 != 0) & (np.abs(d2) < TINY)).mean())
    print("%s: %.4f of the off-diagonal d2 subnormal and non-zero, %.4f zero" % (name, share, float((d2 == 0).mean())))
    assert share >= 0.9
    assert np.all(_ref(name) != 0)
    flushed = _variant(x, lab, flush=True)
    assert not np.array_equal(bits(flushed), bits(_ref(name)))
    assert np.all(flushed == 0)                                           # every distance gone: a = b = 0


@pytest.mark.parametrize("name", ["vanish", "overflow"])
def test_vanish_and_overflow_score_zero_everywhere(name):
    x, _ = hs.rung(name)
    assert np.isfinite(x).all() and np.all(bits(_ref(name)) == 0)
    d2 = _d2(x)[~np.eye(len(x), dtype=bool)]
    print("%s: %.4f of the off-diagonal d2 are +inf, %.4f are 0" % (name, float(np.isinf(d2).mean()), float((d2 == 0).mean())))
    if name == "vanish":
        assert (d2 == 0).mean() > 0.99 and d2.max() <= np.float32(2.0 ** -149)    # a few pairs round up to the last bit
    else:
        assert np.isinf(d2).mean() > 0.5 and not np.isnan(d2).any()


def test_huge_stays_finite():
    d2 = _d2(hs.rung("huge")[0])
    assert np.isfinite(d2).all() and d2.max() > 2.0 ** 120
    assert np.all(_ref("huge") != 0)


def test_far_zeroes_exactly_the_displaced_cluster():
    x, lab = hs.rung("far")
    rows = hs.facts("far")["displaced"]
    assert np.array_equal(rows, np.flatnonzero(lab == hs.FAR_LABEL)) and 30 < len(rows) < 100
    s = _ref("far")
    assert np.array_equal(np.flatnonzero(s == 0), rows)
    d2 = _d2(x)
    other = np.setdiff1d(np.arange(len(x)), rows)
    assert np.all(np.isposinf(d2[np.ix_(rows, other)])) and np.isfinite(d2[np.ix_(rows, rows)]).all()
    assert np.isfinite(d2[np.ix_(other, other)]).all()


def test_scaled_rungs_are_one_grid():
    ints = hs.grid_ints("huge")
    for name in hs.SCALED:
        assert np.array_equal(hs.grid_ints(name), ints) and np.array_equal(hs.rung(name)[1], hs.rung("huge")[1])
    # where nothing under- or overflows, a scaling by 2^e moves no bit of the scores
    x, lab = hs.rung("huge")
    unit = silhouette_samples_ref(np.ldexp(x, -58), lab)
    assert np.array_equal(bits(unit), bits(_ref("huge")))


# ---------------------------------------------------------------------------------------------------------------------
# seams, off-origin plants

@pytest.mark.parametrize("name", hs.SEAMS)
def test_seams_puts_the_boundaries_where_it_says(name):
    _, d, n, variant = name.split("-")
    n = int(n)
    x, lab = hs.rung(name)
    assert x.shape == (n, int(d))
    srt = lab[np.argsort(lab, kind="stable")]
    cuts = list(np.flatnonzero(np.diff(srt)) + 1)
    assert cuts == hs.facts(name)["cuts"] == hs.seam_cuts(n, variant)
    k = len(cuts) + 1
    assert 2 <= k <= n - 1
    if variant == "k2":
        assert k == 2 and cuts == [1]
    elif variant == "kmax":
        assert k == n - 1
        if n > 33:
            assert srt[31] == srt[32]                                     # the one pair lies across the chunk seam
    else:
        want = [c for c in (31, 32, 33, 255, 256, 257) if c < n - 1]
        assert set(want) <= set(cuts)
        assert cuts[0] == 1 and cuts[-1] == n - 1                         # singletons at both ends
        if n > 97:
            assert 64 in cuts and 96 in cuts and not any(64 < c < 96 for c in cuts)      # one whole 32-row chunk
        if n == 1025:
            assert 257 in cuts and 769 in cuts and not any(257 < c < 769 for c in cuts)  # covers block [512, 768)
    if n > 3:
        assert not np.array_equal(lab, srt)                               # shuffled


def test_seams_reaches_every_planted_boundary_somewhere():
    seen = set()
    for name in hs.SEAMS:
        seen |= set(hs.facts(name)["cuts"])
    assert {31, 32, 33, 255, 256, 257} <= seen


def test_offorigin_plants():
    x, lab = hs.rung("offorigin")
    f = hs.facts("offorigin")
    s = _ref("offorigin")
    assert np.abs(x).min() > 2.0 ** 16                                    # far from the origin
    same = f["same"]
    assert len(same) > 20 and np.all(x[same] == x[same[0]]) and np.all(lab[same] == 3)
    assert np.all(bits(s[same]) == bits(np.float32(1)))                   # a = 0 exactly
    da, db = f["dup"]
    assert np.array_equal(x[da], x[db]) and np.all(lab[da] == 0) and np.all(lab[db] == 1)
    assert np.all(s[da] != 0) and np.all(s[db] != 0)
    assert np.count_nonzero(lab == 6) == 1 and lab[299] == 6 and s[299] == 0
    twin = np.flatnonzero(np.all(x == x[299], axis=1))
    assert len(twin) == 2 and lab[twin[0]] == 4
    d2 = _d2(x)
    assert np.all(d2[np.ix_(same, same)] == 0) and np.all(d2[da, db] == 0) and d2[299, twin[0]] == 0


# ---------------------------------------------------------------------------------------------------------------------
# cancel: the condition under which the project's tolerance stands

def test_cancel_moves_by_less_than_a_quarter_of_the_tolerance():
    x, lab = hs.rung("cancel")
    assert x.shape == (1500, 64) and len(np.unique(lab)) == 12 and x.min() > 990
    ref = _ref("cancel").astype(np.float64)
    worst = 0.0
    for seed in range(4):
        p = np.random.default_rng(seed).permutation(64)
        moved = silhouette_samples_ref(np.ascontiguousarray(x[:, p]), lab)
        worst = max(worst, float(np.abs(moved.astype(np.float64) - ref).max()))
    print("cancel: the reference moves by at most %.3g under four permutations of the dimensions" % worst)
    assert worst <= S_TOL / 4


# ---------------------------------------------------------------------------------------------------------------------
# no rung is a field of zeros

@pytest.mark.parametrize("name", [n for n in hs.ALL if n not in ("overflow", "vanish")])
def test_at_most_a_tenth_of_the_scores_are_zero(name):
    assert _zero_share_outside(name, _ref(name)) <= 0.10
