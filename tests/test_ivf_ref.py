"""The inverted-file search without a GPU: tests/ivf_ref.py against an independent float64 brute force on dyadic data
(every step of every chain exact in fp32), its tie rule, and the host logic of ops.IndexIVFFlat on a CPU stand-in
backend whose knn() / ivf_build() / ivf_search() are that reference."""
import numpy as np
import pytest
import torch

from ivf_ref import check_ties, ivf_distances, ivf_lists, ivf_search_ref, ivf_select, tie_case
from knn_ref import knn_ref


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dyadic(seed, n, d, nlist, ntotal):
    """Features k / 8 with |k| <= 8: products and squares are multiples of 1/64 up to 1, and sums of d <= 16 of them
    (and xn + rn - 2 ip) stay below 2^7 at a granularity of 2^-6: exact in fp32 at every step, in either distance form."""
    rng = np.random.default_rng(seed)
    mk = lambda m: (rng.integers(-8, 9, (m, d)) / 8.0).astype(np.float32)
    return mk(n), mk(ntotal), mk(nlist)


def _sq(a, b):
    return ((a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]) ** 2).sum(2)


def _brute(x, stored, cent, nprobe, k):
    lists = np.argmin(_sq(stored, cent), 1)                       # the first minimum: the lowest centroid
    dc, dis = _sq(x, cent), _sq(x, stored)
    D = np.full((x.shape[0], k), np.inf, np.float32)
    I = np.full((x.shape[0], k), -1, np.int64)
    for i in range(x.shape[0]):
        probes = np.argsort(dc[i], kind="stable")[:nprobe]
        rows = np.flatnonzero(np.isin(lists, probes))
        order = rows[np.argsort(dis[i][rows], kind="stable")][:k]  # stable over ascending ids: the lower id first
        D[i, :order.size] = dis[i][order]
        I[i, :order.size] = order
    return lists, D, I


@pytest.mark.parametrize("d,nlist", [(8, 5), (15, 12)])
@pytest.mark.parametrize("n", [3, 25])
def test_reference_agrees_with_the_brute_force_on_dyadic_data(oracle, d, nlist, n):
    x, stored, cent = _dyadic(d + n, n, d, nlist, 200)
    lists = ivf_lists(oracle, stored, cent)
    distances = ivf_distances(oracle, x, stored)
    for nprobe in (1, 3, nlist, nlist + 5):
        for k in (1, 4, 32):
            lb, Db, Ib = _brute(x, stored, cent, nprobe, k)
            assert np.array_equal(lists, lb)
            D, I = ivf_search_ref(oracle, x, stored, lists, cent, nprobe, k, distances=distances)
            assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == (n, k) and I.shape == (n, k)
            assert np.array_equal(I, Ib) and np.array_equal(bits(D), bits(Db)), (nprobe, k)
    Da, Ia = ivf_search_ref(oracle, x, stored, lists, cent, nlist, 10, distances=distances)
    if n >= 20:                                                   # everything probed: the flat search
        Df, If = knn_ref(oracle, x, stored, 10)
        assert np.array_equal(Ia, If) and np.array_equal(bits(Da), bits(Df))
    De, Ie = ivf_search_ref(oracle, x, stored[:0], lists[:0], cent, 2, 3)
    assert np.all(Ie == -1) and np.all(np.isposinf(De)) and Ie.shape == (n, 3)


def test_reference_lists_the_lowest_ids_of_every_tie_group(oracle):
    x, stored, inside, across = tie_case()
    full = _sq(x, stored)                                         # dyadic: exact, equal to the fp32 values
    dis, ok = ivf_distances(oracle, x, stored)
    both = np.tile(np.array([[0, 1]], np.int64), (x.shape[0], 1))
    one = np.tile(np.array([[1, -1]], np.int64), (x.shape[0], 1))
    cut_inside = False
    for k in (1, 19, 20, 21, 32):
        for lists in (inside, across):
            for probes in (both, one):
                D, I = ivf_select(dis, ok, lists, probes, k)
                assert np.all(I >= 0)
                allowed = np.isin(lists, probes[0][probes[0] >= 0])[None, :].repeat(x.shape[0], 0)
                assert np.all(allowed[np.arange(x.shape[0])[:, None], I])
                cut_inside |= check_ties(D, I, full, allowed, k)
    assert cut_inside                                             # the cut at k fell inside a tie group


# ---- ops.IndexIVFFlat on a CPU stand-in ----------------------------------------------------------------------------

def _stand_ins(oracle):
    from oracle_backend import OracleBackend

    class IvfBackend(OracleBackend):
        """knn, ivf_build and ivf_search are the references."""
        built = 0

        def knn(self, x, c, k, want_dist=True):
            D, I = knn_ref(oracle, self._f32(x).numpy(), self._f32(c).numpy(), int(k))
            return torch.from_numpy(I), (torch.from_numpy(D) if want_dist else None)

        def ivf_build(self, rows, lists, nlist):
            self.built += 1
            return {"rows": self._f32(rows).numpy().copy(), "lists": lists.numpy().copy(), "nlist": int(nlist)}

        def ivf_search(self, x, probes, image, k, want_dist=True):
            dis, ok = ivf_distances(oracle, self._f32(x).numpy(), image["rows"])
            D, I = ivf_select(dis, ok, image["lists"], probes.numpy(), int(k))
            return torch.from_numpy(I), (torch.from_numpy(D) if want_dist else None)

    return OracleBackend, IvfBackend


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(33)
    cent = rng.standard_normal((6, 12)).astype(np.float32)
    stored = (cent[rng.integers(0, 6, 150)] + 0.3 * rng.standard_normal((150, 12))).astype(np.float32)
    q = (cent[rng.integers(0, 6, 23)] + 0.3 * rng.standard_normal((23, 12))).astype(np.float32)
    return stored, q, cent


def _index(oracle, cent, backend=None):
    from audio_tokens_amd.ops import IndexFlatL2, IndexIVFFlat
    be = backend or _stand_ins(oracle)[1]()
    quant = IndexFlatL2(cent.shape[1], backend=be)
    if cent.shape[0]:
        quant.add(cent)
    return IndexIVFFlat(quant, cent.shape[1], 6, backend=be)


def test_constructor_and_call_errors(oracle, table):
    import audio_tokens_amd.ops as ops
    from audio_tokens_amd.ops import IndexFlatIP, IndexFlatL2, IndexIVFFlat
    assert "IndexIVFFlat" in ops.__all__
    plain, ivf = _stand_ins(oracle)
    stored, q, cent = table
    with pytest.raises(NotImplementedError, match="knn"):
        IndexIVFFlat(IndexFlatL2(12, backend=plain()), 12, 6)
    with pytest.raises(ValueError):
        IndexIVFFlat(IndexFlatIP(12, backend=ivf()), 12, 6)
    with pytest.raises(ValueError):
        IndexIVFFlat(IndexFlatL2(8, backend=ivf()), 12, 6)
    with pytest.raises(RuntimeError, match="5.*6"):              # a quantiser of another size names both numbers
        _index(oracle, cent[:5])
    index = _index(oracle, cent[:0])
    assert not index.is_trained and index.ntotal == 0 and index.nprobe == 1
    for call in (lambda: index.add(stored), lambda: index.add_core(stored, np.zeros(150, np.int64)),
                 lambda: index.search(q, 3)):
        with pytest.raises(RuntimeError, match="not trained"):
            call()
    index = _index(oracle, cent)
    assert index.is_trained
    for k in (0, -1):
        with pytest.raises(RuntimeError, match="at least 1"):
            index.search(q, k)
    for k in (33, 1000):
        with pytest.raises(NotImplementedError, match="32"):
            index.search(q, k)
    D, I = index.search(q, 5)                                     # an empty index
    assert D.shape == (23, 5) and D.dtype == np.float32 and np.all(np.isposinf(D))
    assert I.shape == (23, 5) and I.dtype == np.int64 and np.all(I == -1)
    index.add(stored)
    for nprobe in (0, -3):
        index.nprobe = nprobe
        with pytest.raises(RuntimeError, match="nprobe"):
            index.search(q, 3)
    index.nprobe = 1
    for wrong in (np.full(150, 6, np.int64), np.full(150, -2, np.int64)):
        with pytest.raises(RuntimeError, match="outside"):
            index.add_core(stored, wrong)
    with pytest.raises(ValueError):
        index.add_core(stored, np.zeros(150, np.int32))
    with pytest.raises(ValueError):
        index.add_core(stored, np.zeros(149, np.int64))
    bad = stored.copy()
    bad[7, 3] = np.nan
    with pytest.raises(RuntimeError, match="input contains NaN's or Inf's"):
        index.add(bad)
    assert index.ntotal == 150                                    # raised before anything was appended
    index.quantizer.add(cent[:1])                                 # the quantiser grew behind the index's back
    with pytest.raises(RuntimeError, match="7.*6"):
        index.search(q, 3)


def test_add_add_core_search_reset(oracle, table):
    _, ivf = _stand_ins(oracle)
    stored, q, cent = table
    lists = ivf_lists(oracle, stored, cent)
    assert np.all(lists >= 0) and len(set(lists.tolist())) == 6
    be = ivf()
    index = _index(oracle, cent, be)
    index.train(stored[:10])                                      # trained already: nothing happens
    assert index.quantizer.ntotal == 6
    index.add(stored)
    assert index.ntotal == 150
    sizes = index.list_sizes
    assert isinstance(sizes, np.ndarray) and sizes.dtype == np.int64
    assert np.array_equal(sizes, np.bincount(lists, minlength=6))
    assert be.built == 0                                          # the image is built at the first search ...
    distances = ivf_distances(oracle, q, stored)
    for nprobe, k in ((1, 1), (1, 10), (3, 4), (6, 32), (11, 10)):
        index.nprobe = nprobe
        D, I = index.search(q, k)                                 # numpy in, numpy out
        assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray) and D.dtype == np.float32 and I.dtype == np.int64
        Dr, Ir = ivf_search_ref(oracle, q, stored, lists, cent, nprobe, k, distances=distances)
        assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr)), (nprobe, k)
    assert be.built == 1                                          # ... and cached
    index.nprobe = 11                                             # above nlist: acts as nlist, the flat search
    Df, If = knn_ref(oracle, q, stored, 10)
    D, I = index.search(q, 10)
    assert np.array_equal(I, If) and np.array_equal(bits(D), bits(Df))
    Dt, It = index.search(torch.from_numpy(q), 10)                # a host tensor is host input: numpy out (device
    assert isinstance(Dt, np.ndarray) and isinstance(It, np.ndarray)   # tensors come back as tensors: test_gpu_ivf.py)
    assert np.array_equal(It, If) and np.array_equal(bits(Dt), bits(Df))
    D64, I64 = index.search(q.astype(np.float64), 10)             # float64: converted first
    assert np.array_equal(I64, If) and np.array_equal(bits(D64), bits(Df))
    D1, I1 = index.search(q)                                      # k = 1 by default
    assert D1.shape == (23, 1) and np.array_equal(I1[:, 0], If[:, 0])

    core = _index(oracle, cent, ivf())                            # the same index from ready list numbers, in two parts
    core.add_core(stored[:70], lists[:70])
    core.add_core(torch.from_numpy(stored[70:]), torch.from_numpy(lists[70:]))
    assert core.ntotal == 150 and np.array_equal(core.list_sizes, sizes)
    for nprobe in (2, 6):
        index.nprobe = core.nprobe = nprobe
        (Da, Ia), (Db, Ib) = index.search(q, 7), core.search(q, 7)
        assert np.array_equal(Ia, Ib) and np.array_equal(bits(Da), bits(Db))
    index.add(stored[:30])                                        # an add drops the image
    assert index.ntotal == 180 and be.built == 1
    index.search(q, 3)
    assert be.built == 2

    index.reset()
    assert index.ntotal == 0 and index.is_trained and index.quantizer.ntotal == 6
    assert np.array_equal(index.list_sizes, np.zeros(6, np.int64))
    assert np.all(index.search(q, 2)[1] == -1)


def test_unlisted_rows_count_and_are_never_found(oracle, table):
    _, ivf = _stand_ins(oracle)
    stored, q, cent = table
    bad = stored.copy()
    bad[[7, 90], [3, 0]] = [np.nan, np.inf]
    lists = ivf_lists(oracle, bad, cent)
    assert lists[7] == -1 and lists[90] == -1 and np.count_nonzero(lists < 0) == 2
    index = _index(oracle, cent)
    index.add(bad, check_finite=False)
    assert index.ntotal == 150 and int(index.list_sizes.sum()) == 148
    index.nprobe = 6
    D, I = index.search(q, 32)
    Dr, Ir = ivf_search_ref(oracle, q, bad, lists, cent, 6, 32)
    assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))
    assert not np.isin(I, [7, 90]).any()
    core = _index(oracle, cent)                                   # a finite row handed in as "no list" is not found either
    given = ivf_lists(oracle, stored, cent)
    given[[4, 5]] = -1
    core.add_core(stored, given)
    core.nprobe = 6
    assert core.ntotal == 150 and int(core.list_sizes.sum()) == 148
    I2 = core.search(q, 32)[1]
    assert not np.isin(I2, [4, 5]).any() and np.all(I2 >= 0)
    qn = q.copy()
    qn[2, 5] = np.nan                                             # a NaN query probes nothing
    I3 = core.search(qn, 4)[1]
    assert np.all(I3[2] == -1) and np.all(I3[[0, 1, 3]] >= 0)


def test_train_fills_an_empty_quantiser(oracle):
    from audio_tokens_amd.ops import Kmeans
    _, ivf = _stand_ins(oracle)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((400, 12)).astype(np.float32)
    be = ivf()
    index = _index(oracle, x[:0], be)
    index.train(x)
    km = Kmeans(12, 6, niter=10, seed=1234, max_points_per_centroid=256, backend=be)
    km.train(x)
    assert index.is_trained and index.quantizer.ntotal == 6
    assert np.array_equal(bits(index.quantizer._c.numpy()), bits(km.centroids))
    index.add(x[:200])
    index.add(x[200:])
    index.nprobe = 2
    D, I = index.search(x[:25], 5)
    lists = ivf_lists(oracle, x, km.centroids)
    assert np.array_equal(index.list_sizes, np.bincount(lists, minlength=6))
    Dr, Ir = ivf_search_ref(oracle, x[:25], x, lists, km.centroids, 2, 5)
    assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))
