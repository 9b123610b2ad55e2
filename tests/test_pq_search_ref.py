"""The search over product-quantiser codes without a GPU: tests/pq_search_ref.py against an independent brute force on
dyadic data (every step of every chain exact in fp32, so plain float64 numpy gives the same values), its tie rule, and
the host logic of ops.IndexPQ on a CPU stand-in backend whose pq_search() is that reference."""
import numpy as np
import pytest
import torch

from pq_ref import pq_decode_ref, pq_encode_ref
from pq_search_ref import pq_search_ref, pq_tables


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dyadic(seed, n, d, M, ksub, ntotal):
    """Features and words k / 8 with |k| <= 8: differences are multiples of 1/8 below 2 in size, squares multiples of
    1/64 up to 4, and a sum of d <= 16 of them stays below 2^7 at a granularity of 2^-6: exact in fp32 at every step."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-8, 9, (n, d)) / 8.0).astype(np.float32)
    cb = (rng.integers(-8, 9, (M, ksub, d // M)) / 8.0).astype(np.float32)
    codes = rng.integers(0, ksub, (ntotal, M)).astype(np.uint8)
    return x, cb, codes


def _brute_distances(x, cb, codes):
    """float64 [n, ntotal]: the squared distance of x[i] to the decoded row r."""
    dec = pq_decode_ref(codes, cb).astype(np.float64)
    return ((x.astype(np.float64)[:, None, :] - dec[None, :, :]) ** 2).sum(2)


def _brute_search(x, cb, codes, k):
    dis = _brute_distances(x, cb, codes)
    n, ntotal = dis.shape
    D = np.full((n, k), np.inf, np.float32)
    I = np.full((n, k), -1, np.int64)
    for i in range(n):
        order = np.argsort(dis[i], kind="stable")[:k]       # stable over ascending ids: the lower id first
        D[i, :order.size] = dis[i][order]
        I[i, :order.size] = order
    return D, I


@pytest.mark.parametrize("d,M,ksub", [(8, 2, 256), (15, 3, 7)])
@pytest.mark.parametrize("n", [3, 25])
def test_reference_agrees_with_the_brute_force_on_dyadic_data(oracle, d, M, ksub, n):
    x, cb, codes_all = _dyadic(d + n, n, d, M, ksub, 300)
    T = pq_tables(oracle, x, cb)
    assert T.dtype == np.float32 and T.shape == (n, M, ksub)
    for ntotal in (0, 1, 9, 300):
        codes = codes_all[:ntotal]
        for k in (1, 4, 128):
            D, I = pq_search_ref(oracle, x, cb, codes, k, tables=T)
            Db, Ib = _brute_search(x, cb, codes, k)
            assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == (n, k) and I.shape == (n, k)
            assert np.array_equal(I, Ib) and np.array_equal(bits(D), bits(Db)), (ntotal, k)
            filled = min(k, ntotal)
            assert np.all(I[:, filled:] == -1) and np.all(np.isposinf(D[:, filled:])) and np.all(I[:, :filled] >= 0)


def test_reference_lists_the_lowest_ids_of_every_tie_group(oracle):
    x, cb, seven = _dyadic(5, 25, 8, 2, 256, 7)
    assert len({tuple(r) for r in seven}) == 7
    codes = np.tile(seven, (40, 1))                          # row r carries code row r % 7
    full = _brute_distances(x, cb, codes)
    T = pq_tables(oracle, x, cb)
    for k in (1, 39, 40, 41, 128):
        D, I = pq_search_ref(oracle, x, cb, codes, k, tables=T)
        assert np.all(I >= 0)
        for i in range(x.shape[0]):
            assert np.all(np.diff(D[i]) >= 0)
            for v in np.unique(D[i]):
                listed, group = I[i][D[i] == v], np.flatnonzero(full[i] == v)
                assert group.size >= 40 and np.array_equal(listed, group[:listed.size]), (k, i, v)
                if v != D[i, -1]:
                    assert listed.size == group.size


def test_codes_outside_the_codebook_and_non_finite_entries_are_never_listed(oracle):
    x, cb, codes = _dyadic(9, 5, 15, 3, 7, 60)
    codes[[3, 17, 59], [0, 1, 2]] = [7, 255, 100]            # >= ksub
    cb[1, 4, 2] = np.nan                                      # the rows that use word 4 of sub-space 1
    x[2, 7] = np.inf
    D, I = pq_search_ref(oracle, x, cb, codes, 60)
    gone = {3, 17, 59} | set(np.flatnonzero(codes[:, 1] == 4).tolist())
    assert np.all(I[2] == -1) and np.all(np.isposinf(D[2]))
    for i in (0, 1, 3, 4):
        assert set(I[i][I[i] >= 0].tolist()) == set(range(60)) - gone


# ---- ops.IndexPQ on a CPU stand-in ---------------------------------------------------------------------------------

def _stand_ins(oracle):
    from oracle_backend import OracleBackend

    class SearchBackend(OracleBackend):
        """pq_search is the reference."""
        def pq_search(self, x, codebooks, codes, k, want_dist=True):
            if isinstance(codes, torch.Tensor):
                codes = codes.numpy()
            D, I = pq_search_ref(oracle, self._f32(x).numpy(), self._f32(codebooks).numpy(), codes, int(k))
            return torch.from_numpy(I), (torch.from_numpy(D) if want_dist else None)

    return OracleBackend, SearchBackend


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(21)
    cb = rng.standard_normal((2, 256, 8)).astype(np.float32)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    q = rng.standard_normal((23, 16)).astype(np.float32)
    return x, q, cb


def test_constructor_and_call_errors(oracle, table):
    from audio_tokens_amd.ops import IndexPQ
    import audio_tokens_amd.ops as ops
    assert "IndexPQ" in ops.__all__
    plain, search = _stand_ins(oracle)
    x, q, cb = table
    with pytest.raises(ValueError):
        IndexPQ(16, 3, backend=search())
    with pytest.raises(NotImplementedError, match="nbits"):
        IndexPQ(16, 2, nbits=4, backend=search())
    with pytest.raises(NotImplementedError, match="64"):
        IndexPQ(130, 65, backend=search())
    with pytest.raises(NotImplementedError, match="pq_search"):
        IndexPQ(16, 2, backend=plain())
    index = IndexPQ(128, 64, backend=search())                # the largest M is accepted
    index = IndexPQ(16, 2, backend=search())
    assert not index.is_trained and index.ntotal == 0
    with pytest.raises(RuntimeError, match="not trained"):
        index.search(q, 3)
    with pytest.raises(RuntimeError, match="not trained"):
        index.add(x)
    index.pq.set_centroids(cb)
    assert index.is_trained
    for k in (0, -1):
        with pytest.raises(RuntimeError, match="at least 1"):
            index.search(q, k)
    for k in (129, 1000):
        with pytest.raises(NotImplementedError, match="128"):
            index.search(q, k)
    D, I = index.search(q, 5)                                 # an empty index
    assert D.shape == (23, 5) and D.dtype == np.float32 and np.all(np.isposinf(D))
    assert I.shape == (23, 5) and I.dtype == np.int64 and np.all(I == -1)
    bad = x.copy()
    bad[7, 3] = np.nan
    with pytest.raises(RuntimeError, match="input contains NaN's or Inf's"):
        index.add(bad)
    assert index.ntotal == 0                                  # raised before anything was appended
    index.add(bad, check_finite=False)
    assert index.ntotal == 300 and index.codes[7, 0] == 0
    with pytest.raises(RuntimeError, match="reconstruct_n"):
        index.reconstruct_n(200, 101)


def test_add_search_reconstruct_reset(oracle, table):
    from audio_tokens_amd.ops import IndexPQ
    _, search = _stand_ins(oracle)
    x, q, cb = table
    cr = pq_encode_ref(oracle, x, cb)[0]
    Dr, Ir = pq_search_ref(oracle, q, cb, cr, 10)
    index = IndexPQ(16, 2, backend=search())
    index.pq.set_centroids(cb)
    index.add(x)
    assert index.ntotal == 300 and isinstance(index.codes, torch.Tensor) and index.codes.dtype == torch.uint8
    assert np.array_equal(index.codes.numpy(), cr)
    D, I = index.search(q, 10)                                # numpy in, numpy out
    assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray) and D.dtype == np.float32 and I.dtype == np.int64
    assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))
    D1, I1 = index.search(q)                                  # k = 1 by default: column 0
    assert D1.shape == (23, 1) and np.array_equal(I1[:, 0], Ir[:, 0]) and np.array_equal(bits(D1[:, 0]), bits(Dr[:, 0]))

    parts = IndexPQ(16, 2, backend=search())                  # in two parts, host and "device" (20 rows or more each:
    parts.pq.set_centroids(cb)                                # the encoder's distance form is chosen by the call)
    parts.add(x[:140])
    assert parts.ntotal == 140
    parts.add(torch.from_numpy(x[140:]))
    assert parts.ntotal == 300 and np.array_equal(parts.codes.numpy(), cr)
    D2, I2 = parts.search(q, 10)
    assert np.array_equal(I2, Ir) and np.array_equal(bits(D2), bits(Dr))

    D3, I3 = index.search(q.astype(np.float64), 10)           # float64: converted first
    assert np.array_equal(I3, Ir) and np.array_equal(bits(D3), bits(Dr))
    wide = np.zeros((23, 32), np.float32)
    wide[:, ::2] = q
    D4, I4 = index.search(wide[:, ::2], 10)                   # strided
    assert np.array_equal(I4, Ir) and np.array_equal(bits(D4), bits(Dr))
    tall = torch.zeros((46, 16))
    tall[::2] = torch.from_numpy(q)
    D5, I5 = index.search(tall[::2], 10)
    assert np.array_equal(I5, Ir) and np.array_equal(bits(D5), bits(Dr))

    dec = index.pq.decode(cr)
    assert np.array_equal(bits(index.reconstruct_n(0, 300)), bits(dec))
    assert np.array_equal(bits(index.reconstruct_n(17, 5)), bits(dec[17:22]))
    assert np.array_equal(bits(index.reconstruct_n(290)), bits(dec[290:]))
    assert np.array_equal(bits(index.reconstruct(123)), bits(dec[123])) and index.reconstruct(123).shape == (16,)
    assert np.array_equal(bits(dec), bits(pq_decode_ref(cr, cb)))

    index.reset()
    assert index.ntotal == 0 and index.is_trained and tuple(index.codes.shape) == (0, 2)
    assert np.all(index.search(q, 2)[1] == -1)
    index.add_codes(cr[:100])                                 # ready codes, host and "device"
    index.add_codes(torch.from_numpy(cr[100:]))
    assert index.ntotal == 300 and np.array_equal(index.codes.numpy(), cr)
    D6, I6 = index.search(q, 10)
    assert np.array_equal(I6, Ir) and np.array_equal(bits(D6), bits(Dr))
    with pytest.raises(AssertionError):
        index.add_codes(cr[:, :1])
    with pytest.raises(AssertionError):
        index.add_codes(cr.astype(np.int32))


def test_train_is_the_product_quantisers(oracle):
    from audio_tokens_amd.ops import IndexPQ, ProductQuantizer
    _, search = _stand_ins(oracle)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((600, 16)).astype(np.float32)
    index = IndexPQ(16, 2, niter=3, backend=search())
    index.train(x)
    pq = ProductQuantizer(16, 2, niter=3, backend=search())
    pq.train(x)
    assert index.is_trained and np.array_equal(bits(index.pq.centroids), bits(pq.centroids))
    index.add(x[:200])
    index.add(x[200:])
    assert np.array_equal(index.codes.numpy(), pq.compute_codes(x))
    D, I = index.search(x[:5], 3)
    Dr, Ir = pq_search_ref(oracle, x[:5], pq.centroids, pq.compute_codes(x), 3)
    assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))
