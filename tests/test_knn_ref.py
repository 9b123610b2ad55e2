"""tests/knn_ref.py (the bit reference of IndexFlatL2.search(x, k)) on hand-made cases, and the Python-side checks of
search(x, k) on the CPU oracle backend."""
import numpy as np
import pytest

from knn_ref import knn_ref
from oracle_backend import OracleBackend


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _unit(rng, n, d, oracle):
    return oracle.l2norm_rows(rng.standard_normal((n, d)).astype(np.float32))


def _sorted_lex(D, I):
    listed = I >= 0
    for i in range(D.shape[0]):
        m = int(listed[i].sum())
        assert listed[i, :m].all() and not listed[i, m:].any()          # listed entries first, then padding
        assert np.all(np.isinf(D[i, m:])) and np.all(I[i, m:] == -1)
        d, j = D[i, :m], I[i, :m]
        assert np.all((d[1:] > d[:-1]) | ((d[1:] == d[:-1]) & (j[1:] > j[:-1])))


@pytest.mark.parametrize("n", [7, 40])          # the direct form (n < 20) and the product form
def test_column_zero_is_the_nearest_centroid(oracle, n):
    rng = np.random.default_rng(n)
    x, c = _unit(rng, n, 16, oracle), _unit(rng, 30, 16, oracle)
    D, I = knn_ref(oracle, x, c, 6)
    ids, dis = oracle.assign(x, c)
    assert np.array_equal(I[:, 0], ids) and np.array_equal(bits(D[:, 0]), bits(dis))
    _sorted_lex(D, I)


@pytest.mark.parametrize("n", [5, 25])
def test_duplicates_and_rows_on_centroids(oracle, n):
    rng = np.random.default_rng(3 + n)
    c = _unit(rng, 12, 8, oracle)
    c[[4, 9, 11]] = c[2]                            # four copies of one centroid
    x = _unit(rng, n, 8, oracle)
    x[0] = c[2]                                     # a row on the duplicated centroid: four exact zeros
    x[1] = c[7]
    D, I = knn_ref(oracle, x, c, 5)
    assert list(I[0, :4]) == [2, 4, 9, 11] and np.all(bits(D[0, :4]) == 0)
    assert I[1, 0] == 7 and bits(D[1, 0]) == 0
    _sorted_lex(D, I)
    # every row: the tied copies appear together, lower index first
    for i in range(n):
        pos = [list(I[i]).index(j) for j in (2, 4, 9, 11) if j in I[i]]
        assert pos == sorted(pos)


def test_more_than_k_c_and_bad_rows(oracle):
    rng = np.random.default_rng(5)
    n, kc = 24, 6
    x, c = _unit(rng, n, 8, oracle), _unit(rng, kc, 8, oracle)
    x[3, 2] = np.nan                                # NaN row: nothing listed
    x[4] = 3e38                                     # |x|^2 overflows: every distance is +inf or NaN
    D, I = knn_ref(oracle, x, c, kc + 3)
    assert D.shape == (n, kc + 3) and D.dtype == np.float32 and I.dtype == np.int64
    for i in (3, 4):
        assert np.all(I[i] == -1) and np.all(np.isposinf(D[i]))
    good = np.ones(n, bool)
    good[[3, 4]] = False
    assert np.all(I[good, :kc] >= 0) and np.all(I[good, kc:] == -1) and np.all(np.isposinf(D[good, kc:]))
    assert np.array_equal(np.sort(I[good, :kc], 1), np.tile(np.arange(kc), (good.sum(), 1)))
    _sorted_lex(D, I)


def test_search_k_validation_on_the_oracle_backend():
    from audio_tokens_amd.ops import IndexFlatL2
    index = IndexFlatL2(8, backend=OracleBackend())
    index.add(np.eye(8, dtype=np.float32))
    x = np.ones((3, 8), np.float32)
    for bad in (0, -2):
        with pytest.raises(RuntimeError):
            index.search(x, bad)
    with pytest.raises(NotImplementedError):     # k >= 2 needs a backend with knn()
        index.search(x, 5)
    D, I = index.search(x, 1)
    assert D.shape == (3, 1) and I.shape == (3, 1)
