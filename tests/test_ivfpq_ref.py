"""PQ codes behind inverted lists without a GPU: tests/ivfpq_ref.py against an independent float64 brute force on dyadic
data (every step of every chain exact in fp32), its tie rule, and the host logic of ops.IndexIVFPQ on a CPU stand-in
backend whose knn() / ivfpq_build() / ivfpq_search() are that reference."""
import numpy as np
import pytest
import torch

from ivf_ref import check_ties, ivf_lists, ivf_probes, tie_case
from ivfpq_ref import ivfpq_distances, ivfpq_encoder_input, ivfpq_search_ref
from knn_ref import knn_ref
from pq_ref import pq_decode_ref, pq_encode_ref
from pq_search_ref import pq_search_ref


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dyadic(seed, n, d, M, ksub, nlist, ntotal):
    """Features, centroids and words k / 8 with |k| <= 8: a residual is a multiple of 1/8 up to 2 in size, its difference
    with a word up to 3, the squares multiples of 1/64 up to 9, and a sum of d <= 15 of them stays below 2^8 at a
    granularity of 2^-6: exact in fp32 at every step."""
    rng = np.random.default_rng(seed)
    mk = lambda *shape: (rng.integers(-8, 9, shape) / 8.0).astype(np.float32)
    x, cent, cb = mk(n, d), mk(nlist, d), mk(M, ksub, d // M)
    codes = rng.integers(0, ksub, (ntotal, M)).astype(np.uint8)
    lists = rng.integers(0, nlist, ntotal).astype(np.int64)
    return x, cent, cb, codes, lists


def _brute_distances(x, cent, cb, codes, lists, by_residual):
    """float64 [n, ntotal]: the plain squared distance of x[i] to the decoded row r (plus its centroid)."""
    dec = pq_decode_ref(codes, cb).astype(np.float64)
    if by_residual:
        dec = dec + cent.astype(np.float64)[np.maximum(lists, 0)]
    return ((x.astype(np.float64)[:, None, :] - dec[None, :, :]) ** 2).sum(2)


def _brute(x, cent, cb, codes, lists, by_residual, nprobe, k):
    dis = _brute_distances(x, cent, cb, codes, lists, by_residual)
    dc = ((x.astype(np.float64)[:, None, :] - cent.astype(np.float64)[None, :, :]) ** 2).sum(2)
    D = np.full((x.shape[0], k), np.inf, np.float32)
    I = np.full((x.shape[0], k), -1, np.int64)
    for i in range(x.shape[0]):
        probes = np.argsort(dc[i], kind="stable")[:nprobe]
        rows = np.flatnonzero(np.isin(lists, probes))
        order = rows[np.argsort(dis[i][rows], kind="stable")][:k]  # stable over ascending ids: the lower id first
        D[i, :order.size] = dis[i][order]
        I[i, :order.size] = order
    return D, I


@pytest.mark.parametrize("by_residual", [True, False])
@pytest.mark.parametrize("nlist", [3, 7])
@pytest.mark.parametrize("d,M,ksub", [(8, 2, 256), (15, 3, 7)])
def test_reference_agrees_with_the_brute_force_on_dyadic_data(oracle, d, M, ksub, nlist, by_residual):
    n = 21
    x, cent, cb, codes_all, lists_all = _dyadic(d + nlist, n, d, M, ksub, nlist, 300)
    full = ivfpq_distances(oracle, x, cb, codes_all, lists_all, cent, by_residual)
    for ntotal in (0, 1, 9, 300):
        codes, lists = codes_all[:ntotal], lists_all[:ntotal]
        distances = (full[0][:, :ntotal], full[1][:, :ntotal])
        for nprobe in (1, 2, nlist):
            for k in (1, 4, 128):
                D, I = ivfpq_search_ref(oracle, x, cb, codes, lists, cent, nprobe, k, by_residual,
                                        distances=distances if ntotal else None)
                Db, Ib = _brute(x, cent, cb, codes, lists, by_residual, nprobe, k)
                assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == (n, k) and I.shape == (n, k)
                assert np.array_equal(I, Ib) and np.array_equal(bits(D), bits(Db)), (ntotal, nprobe, k)
    # the distances of the probed pairs alone give the same rows
    D1, I1 = ivfpq_search_ref(oracle, x, cb, codes_all, lists_all, cent, 2, 4, by_residual)
    D2, I2 = ivfpq_search_ref(oracle, x, cb, codes_all, lists_all, cent, 2, 4, by_residual, distances=full)
    assert np.array_equal(I1, I2) and np.array_equal(bits(D1), bits(D2))
    if not by_residual:                                           # everything probed, no residual: the search over all codes
        Da, Ia = ivfpq_search_ref(oracle, x, cb, codes_all, lists_all, cent, nlist, 10, False, distances=full)
        Dp, Ip = pq_search_ref(oracle, x, cb, codes_all, 10)
        assert np.array_equal(Ia, Ip) and np.array_equal(bits(Da), bits(Dp))


def tie_codes():
    """tie_case()'s layout over codes: seven distinct code rows, each stored 40 times (row r carries code row r % 7);
    dyadic codebooks, so equal code rows of one list -- and, without residuals, of any list -- are at equal distances."""
    x, stored, inside, across = tie_case()
    rng = np.random.default_rng(6)
    cb = (rng.integers(-8, 9, (2, 256, 4)) / 8.0).astype(np.float32)
    seven = rng.integers(0, 256, (7, 2)).astype(np.uint8)
    assert len({tuple(r) for r in seven}) == 7
    cent = np.zeros((2, 8), np.float32)
    cent[1, 0] = 0.125                                            # two lists, both probed with nprobe = 2
    return x, cb, np.tile(seven, (40, 1)), cent, inside, across


TIE_CASES = (("inside", True), ("inside", False), ("across", False))
TIE_KS = (1, 19, 20, 21, 40, 41, 128)


def test_reference_lists_the_lowest_ids_of_every_tie_group(oracle):
    x, cb, codes, cent, inside, across = tie_codes()
    assert np.all(ivf_probes(oracle, x, cent, 2) >= 0)
    for which, by_residual in TIE_CASES:
        lists = inside if which == "inside" else across
        full = _brute_distances(x, cent, cb, codes, lists, by_residual)   # dyadic: exact, equal to the fp32 values
        distances = ivfpq_distances(oracle, x, cb, codes, lists, cent, by_residual)
        allowed = np.ones(full.shape, bool)
        cut_inside = False
        for k in TIE_KS:
            D, I = ivfpq_search_ref(oracle, x, cb, codes, lists, cent, 2, k, by_residual, distances=distances)
            assert np.all(I >= 0)
            cut_inside |= check_ties(D, I, full, allowed, k)
        assert cut_inside, (which, by_residual)                   # the cut at k fell inside a tie group
        if which == "across":                                     # a tie group spans both lists
            D, I = ivfpq_search_ref(oracle, x, cb, codes, lists, cent, 2, 40, False, distances=distances)
            for i in range(x.shape[0]):
                nearest = lists[I[i][D[i] == D[i, 0]]]
                assert (nearest == 0).any() and (nearest == 1).any()


# ---- ops.IndexIVFPQ on a CPU stand-in ------------------------------------------------------------------------------

def _stand_ins(oracle):
    from oracle_backend import OracleBackend

    class IvfpqBackend(OracleBackend):
        """knn, ivfpq_build and ivfpq_search are the references."""
        built = 0

        def knn(self, x, c, k, want_dist=True):
            D, I = knn_ref(oracle, self._f32(x).numpy(), self._f32(c).numpy(), int(k))
            return torch.from_numpy(I), (torch.from_numpy(D) if want_dist else None)

        def ivfpq_build(self, codes, lists, nlist):
            self.built += 1
            return {"codes": codes.numpy().copy(), "lists": lists.numpy().copy(), "nlist": int(nlist)}

        def ivfpq_search(self, x, probes, centroids, codebooks, image, k, want_dist=True):
            cent = None if centroids is None else self._f32(centroids).numpy()
            D, I = ivfpq_search_ref(oracle, self._f32(x).numpy(), self._f32(codebooks).numpy(), image["codes"],
                                    image["lists"], cent, probes.shape[1], int(k), cent is not None, probes=probes.numpy())
            return torch.from_numpy(I), (torch.from_numpy(D) if want_dist else None)

    return OracleBackend, IvfpqBackend


D_, M_, NLIST = 8, 2, 6


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(34)
    cent = rng.standard_normal((NLIST, D_)).astype(np.float32)
    stored = (cent[rng.integers(0, NLIST, 150)] + 0.3 * rng.standard_normal((150, D_))).astype(np.float32)
    q = (cent[rng.integers(0, NLIST, 23)] + 0.3 * rng.standard_normal((23, D_))).astype(np.float32)
    cb = (0.3 * rng.standard_normal((M_, 256, D_ // M_))).astype(np.float32)
    return stored, q, cent, cb


def _index(oracle, cent, cb=None, by_residual=True, backend=None):
    from audio_tokens_amd.ops import IndexFlatL2, IndexIVFPQ
    be = backend or _stand_ins(oracle)[1]()
    quant = IndexFlatL2(D_, backend=be)
    if cent.shape[0]:
        quant.add(cent)
    index = IndexIVFPQ(quant, D_, NLIST, M_, by_residual=by_residual, backend=be)
    if cb is not None:
        index.pq.set_centroids(cb)
    return index


def test_constructor_and_call_errors(oracle, table):
    import audio_tokens_amd.ops as ops
    from audio_tokens_amd.ops import IndexFlatIP, IndexFlatL2, IndexIVFPQ
    assert "IndexIVFPQ" in ops.__all__
    plain, ivfpq = _stand_ins(oracle)
    stored, q, cent, cb = table
    with pytest.raises(NotImplementedError, match="ivfpq_build|knn"):
        IndexIVFPQ(IndexFlatL2(D_, backend=plain()), D_, NLIST, M_)
    with pytest.raises(ValueError):
        IndexIVFPQ(IndexFlatIP(D_, backend=ivfpq()), D_, NLIST, M_)
    with pytest.raises(ValueError):
        IndexIVFPQ(IndexFlatL2(12, backend=ivfpq()), D_, NLIST, M_)
    with pytest.raises(ValueError):
        IndexIVFPQ(IndexFlatL2(D_, backend=ivfpq()), D_, 0, M_)
    with pytest.raises(ValueError):                               # d % M: the quantiser's own error
        IndexIVFPQ(IndexFlatL2(D_, backend=ivfpq()), D_, NLIST, 3)
    with pytest.raises(NotImplementedError, match="nbits"):
        IndexIVFPQ(IndexFlatL2(D_, backend=ivfpq()), D_, NLIST, M_, nbits=4)
    with pytest.raises(NotImplementedError, match="64"):
        IndexIVFPQ(IndexFlatL2(130, backend=ivfpq()), 130, NLIST, 65)
    with pytest.raises(NotImplementedError, match="lists"):
        IndexIVFPQ(IndexFlatL2(D_, backend=ivfpq()), D_, (1 << 24) + 1, M_)
    IndexIVFPQ(IndexFlatL2(128, backend=ivfpq()), 128, NLIST, 64)   # the largest M is accepted
    with pytest.raises(RuntimeError, match="5.*6"):              # a quantiser of another size names both numbers
        _index(oracle, cent[:5])
    for index in (_index(oracle, cent[:0], cb), _index(oracle, cent)):   # no coarse centroids / no codebooks
        assert not index.is_trained and index.ntotal == 0 and index.nprobe == 1 and index.by_residual
        for call in (lambda: index.add(stored), lambda: index.add_core(stored, np.zeros(150, np.int64)),
                     lambda: index.search(q, 3)):
            with pytest.raises(RuntimeError, match="not trained"):
                call()
    index = _index(oracle, cent, cb)
    assert index.is_trained
    for k in (0, -1):
        with pytest.raises(RuntimeError, match="at least 1"):
            index.search(q, k)
    for k in (129, 1000):
        with pytest.raises(NotImplementedError, match="128"):
            index.search(q, k)
    D, I = index.search(q, 5)                                     # an empty index
    assert D.shape == (23, 5) and D.dtype == np.float32 and np.all(np.isposinf(D))
    assert I.shape == (23, 5) and I.dtype == np.int64 and np.all(I == -1)
    assert tuple(index.codes.shape) == (0, M_) and index.codes.dtype == torch.uint8
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
    for i0, n in ((-1, 2), (149, 2), (151, 0)):
        with pytest.raises(RuntimeError, match="reconstruct_n"):
            index.reconstruct_n(i0, n)
    index.quantizer.add(cent[:1])                                 # the quantiser grew behind the index's back
    with pytest.raises(RuntimeError, match="7.*6"):
        index.search(q, 3)


@pytest.mark.parametrize("by_residual", [True, False])
def test_add_add_core_search_reconstruct_reset(oracle, table, by_residual):
    _, ivfpq = _stand_ins(oracle)
    stored, q, cent, cb = table
    lists = ivf_lists(oracle, stored, cent)
    assert np.all(lists >= 0) and len(set(lists.tolist())) == NLIST
    codes, _, bad = pq_encode_ref(oracle, ivfpq_encoder_input(stored, lists, cent, by_residual), cb)
    assert not bad
    be = ivfpq()
    index = _index(oracle, cent, cb, by_residual, be)
    assert index.by_residual == by_residual
    index.add(stored)
    assert index.ntotal == 150 and isinstance(index.codes, torch.Tensor) and index.codes.dtype == torch.uint8
    assert np.array_equal(index.codes.numpy(), codes)
    sizes = index.list_sizes
    assert isinstance(sizes, np.ndarray) and sizes.dtype == np.int64
    assert np.array_equal(sizes, np.bincount(lists, minlength=NLIST))
    assert be.built == 0                                          # the image is built at the first search ...
    distances = ivfpq_distances(oracle, q, cb, codes, lists, cent, by_residual)
    for nprobe, k in ((1, 1), (1, 10), (3, 4), (6, 128), (11, 10)):
        index.nprobe = nprobe
        D, I = index.search(q, k)                                 # numpy in, numpy out
        assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray) and D.dtype == np.float32 and I.dtype == np.int64
        Dr, Ir = ivfpq_search_ref(oracle, q, cb, codes, lists, cent, nprobe, k, by_residual, distances=distances)
        assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr)), (nprobe, k)
    assert be.built == 1                                          # ... and cached
    index.nprobe = 11                                             # above nlist: acts as nlist
    Df, If = ivfpq_search_ref(oracle, q, cb, codes, lists, cent, NLIST, 10, by_residual, distances=distances)
    if not by_residual:                                           # ... which without residuals is the search over all codes
        Dp, Ip = pq_search_ref(oracle, q, cb, codes, 10)
        assert np.array_equal(If, Ip) and np.array_equal(bits(Df), bits(Dp))
    Dt, It = index.search(torch.from_numpy(q), 10)                # a host tensor is host input: numpy out
    assert isinstance(Dt, np.ndarray) and isinstance(It, np.ndarray)
    assert np.array_equal(It, If) and np.array_equal(bits(Dt), bits(Df))
    D64, I64 = index.search(q.astype(np.float64), 10)             # float64: converted first
    assert np.array_equal(I64, If) and np.array_equal(bits(D64), bits(Df))
    wide = np.zeros((23, 2 * D_), np.float32)
    wide[:, ::2] = q
    Ds, Is = index.search(wide[:, ::2], 10)                       # strided input
    assert np.array_equal(Is, If) and np.array_equal(bits(Ds), bits(Df))
    D1, I1 = index.search(q)                                      # k = 1 by default
    assert D1.shape == (23, 1) and np.array_equal(I1[:, 0], If[:, 0])

    rec = index.reconstruct_n(0, 150)                             # decode, plus the centroid in one fp32 addition
    want = pq_decode_ref(codes, cb)
    if by_residual:
        want = want + cent[lists]
    assert isinstance(rec, np.ndarray) and rec.dtype == np.float32 and np.array_equal(bits(rec), bits(want))
    assert np.array_equal(bits(index.reconstruct_n(40, 3)), bits(want[40:43]))
    assert np.array_equal(bits(index.reconstruct_n(147)), bits(want[147:]))
    assert np.array_equal(bits(index.reconstruct(5)), bits(want[5])) and index.reconstruct_n(150, 0).shape == (0, D_)

    core = _index(oracle, cent, cb, by_residual, ivfpq())         # the same index from ready list numbers, in two parts
    core.add_core(stored[:70], lists[:70])
    core.add_core(torch.from_numpy(stored[70:]), torch.from_numpy(lists[70:]))
    parts = _index(oracle, cent, cb, by_residual, ivfpq())        # ... and from two adds
    parts.add(stored[:70].astype(np.float64))
    parts.add(stored[70:])
    for other in (core, parts):
        assert other.ntotal == 150 and np.array_equal(other.list_sizes, sizes)
        assert np.array_equal(other.codes.numpy(), codes)
        for nprobe in (2, 6):
            index.nprobe = other.nprobe = nprobe
            (Da, Ia), (Db, Ib) = index.search(q, 7), other.search(q, 7)
            assert np.array_equal(Ia, Ib) and np.array_equal(bits(Da), bits(Db))
    index.add(stored[:30])                                        # an add drops the image
    assert index.ntotal == 180 and be.built == 1
    index.search(q, 3)
    assert be.built == 2

    index.reset()
    assert index.ntotal == 0 and index.is_trained and index.quantizer.ntotal == NLIST and index.pq.is_trained
    assert np.array_equal(index.list_sizes, np.zeros(NLIST, np.int64)) and tuple(index.codes.shape) == (0, M_)
    assert np.all(index.search(q, 2)[1] == -1)


@pytest.mark.parametrize("by_residual", [True, False])
def test_unlisted_rows_count_and_are_never_found(oracle, table, by_residual):
    stored, q, cent, cb = table
    bad = stored.copy()
    bad[[7, 90], [3, 0]] = [np.nan, np.inf]
    lists = ivf_lists(oracle, bad, cent)
    assert lists[7] == -1 and lists[90] == -1 and np.count_nonzero(lists < 0) == 2
    index = _index(oracle, cent, cb, by_residual)
    index.add(bad, check_finite=False)
    assert index.ntotal == 150 and int(index.list_sizes.sum()) == 148
    codes, _, flag = pq_encode_ref(oracle, ivfpq_encoder_input(bad, lists, cent, by_residual), cb)
    assert not flag and np.array_equal(index.codes.numpy(), codes)   # a row of list -1 is encoded from a zero vector
    index.nprobe = NLIST
    D, I = index.search(q, 128)
    Dr, Ir = ivfpq_search_ref(oracle, q, cb, codes, lists, cent, NLIST, 128, by_residual)
    assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))
    assert not np.isin(I, [7, 90]).any() and np.all(I >= 0)
    rec = index.reconstruct_n()
    assert np.all(np.isnan(rec[[7, 90]])) and np.all(np.isfinite(np.delete(rec, [7, 90], 0)))
    core = _index(oracle, cent, cb, by_residual)                  # a finite row handed in as "no list" is not found either
    given = ivf_lists(oracle, stored, cent)
    given[[4, 5]] = -1
    core.add_core(stored, given)
    core.nprobe = NLIST
    assert core.ntotal == 150 and int(core.list_sizes.sum()) == 148
    I2 = core.search(q, 128)[1]
    assert not np.isin(I2, [4, 5]).any() and np.all(np.isnan(core.reconstruct_n(4, 2)))
    qn = q.copy()
    qn[2, 5] = np.nan                                             # a NaN query probes nothing
    I3 = core.search(qn, 4)[1]
    assert np.all(I3[2] == -1) and np.all(I3[[0, 1, 3]] >= 0)


@pytest.mark.parametrize("by_residual", [True, False])
def test_train_trains_both_quantisers(oracle, by_residual):
    from audio_tokens_amd.ops import Kmeans, ProductQuantizer
    _, ivfpq = _stand_ins(oracle)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((700, D_)).astype(np.float32)
    be = ivfpq()
    from audio_tokens_amd.ops import IndexFlatL2, IndexIVFPQ
    index = IndexIVFPQ(IndexFlatL2(D_, backend=be), D_, NLIST, M_, by_residual=by_residual, niter=2, seed=77, backend=be)
    assert not index.is_trained
    index.train(x)
    km = Kmeans(D_, NLIST, niter=10, seed=1234, max_points_per_centroid=256, backend=be)
    km.train(x)
    assert index.is_trained and index.quantizer.ntotal == NLIST
    cent = km.centroids
    assert np.array_equal(bits(index.quantizer._c.numpy()), bits(cent))
    lists = ivf_lists(oracle, x, cent)
    pq = ProductQuantizer(D_, M_, niter=2, seed=77, backend=be)
    pq.train((x - cent[lists]).astype(np.float32) if by_residual else x)
    assert np.array_equal(bits(index.pq.centroids), bits(pq.centroids))
    ready = IndexIVFPQ(index.quantizer, D_, NLIST, M_, by_residual=by_residual, niter=2, seed=77, backend=be)
    ready.train(x)                                                # a full quantiser is kept; the codebooks are trained
    assert ready.quantizer.ntotal == NLIST and np.array_equal(bits(ready.pq.centroids), bits(pq.centroids))
    index.add(x[:300])
    index.add(x[300:])
    index.nprobe = 2
    D, I = index.search(x[:25], 5)
    codes, _, _ = pq_encode_ref(oracle, ivfpq_encoder_input(x, lists, cent, by_residual), pq.centroids)
    assert np.array_equal(index.codes.numpy(), codes)
    Dr, Ir = ivfpq_search_ref(oracle, x[:25], pq.centroids, codes, lists, cent, 2, 5, by_residual)
    assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))
