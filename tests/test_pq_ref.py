"""Host logic of audio_tokens_amd.ops.ProductQuantizer driven with the CPU stand-in backend (one assign per sub-space,
decode by indexing), against the oracle and tests/pq_ref.py: no GPU involved."""
import numpy as np
import pytest
import torch

from pq_ref import pq_decode_ref, pq_encode_ref


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture()
def cpu_be():
    from oracle_backend import OracleBackend
    return OracleBackend()


@pytest.fixture(scope="module")
def table():
    """x [1000, 16] and random codebooks for M = 4."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1000, 16)).astype(np.float32)
    cb = rng.standard_normal((4, 256, 4)).astype(np.float32)
    cb[:, 200] = cb[:, 3]                                  # duplicate rows: the lower index wins
    x[10:20, 4:8] = cb[1, 3]
    return x, cb


def test_exported():
    from audio_tokens_amd import ops
    assert "ProductQuantizer" in ops.__all__


def test_train_is_one_kmeans_per_subspace(cpu_be, oracle, table):
    from audio_tokens_amd.ops import ProductQuantizer
    x, _ = table
    pq = ProductQuantizer(16, 4, backend=cpu_be)
    assert (pq.d, pq.M, pq.nbits, pq.dsub, pq.ksub, pq.code_size) == (16, 4, 8, 4, 256, 4)
    assert not pq.is_trained and pq.centroids is None
    pq.train(x)                                            # (n < 39 * 256: Kmeans's warning goes to stderr)
    assert pq.is_trained and pq.centroids.shape == (4, 256, 4) and pq.centroids.dtype == np.float32
    assert tuple(pq.centroids_device.shape) == (4, 256, 4)
    for m in range(4):
        want = oracle.kmeans_train(np.ascontiguousarray(x[:, 4 * m:4 * m + 4]), 256, niter=25).centroids
        assert np.array_equal(bits(pq.centroids[m]), bits(want)), m


def test_train_subsamples_every_subspace_with_the_same_permutation(cpu_be, oracle, table):
    from audio_tokens_amd.ops import Kmeans, ProductQuantizer
    x, _ = table
    pq = ProductQuantizer(16, 4, niter=6, max_points_per_centroid=2, backend=cpu_be)
    pq.train(x)
    perm = cpu_be.rand_perm_prefix(1000, 1234, 512)        # faiss: rand_perm(n, seed)[:k * max_points_per_centroid]
    assert len(np.unique(perm)) == 512
    for m in range(4):
        xm = np.ascontiguousarray(x[:, 4 * m:4 * m + 4])
        want = oracle.kmeans_train(xm[perm], 256, niter=6).centroids
        assert np.array_equal(bits(pq.centroids[m]), bits(want)), m
        km = Kmeans(4, 256, niter=6, seed=1234, max_points_per_centroid=2, backend=cpu_be)
        km.train(xm)
        assert np.array_equal(bits(pq.centroids[m]), bits(km.centroids)), m


def test_train_passes_kmeans_errors_and_warning_through(cpu_be, capsys):
    from audio_tokens_amd.ops import ProductQuantizer
    rng = np.random.default_rng(1)
    pq = ProductQuantizer(8, 2, niter=2, backend=cpu_be)
    with pytest.raises(RuntimeError, match="should be at least as large as number of clusters"):
        pq.train(rng.standard_normal((100, 8)).astype(np.float32))
    x = rng.standard_normal((300, 8)).astype(np.float32)
    x[7, 5] = np.nan
    with pytest.raises(RuntimeError, match="NaN's or Inf's"):
        pq.train(x)
    assert not pq.is_trained
    x[7, 5] = 0.0
    capsys.readouterr()
    pq.train(x)
    assert "WARNING clustering 300 points to 256 centroids" in capsys.readouterr().err
    assert pq.is_trained


@pytest.mark.parametrize("n", [1000, 19, 1, 0])
def test_encode_and_decode_against_the_reference(cpu_be, oracle, table, n):
    from audio_tokens_amd.ops import ProductQuantizer
    x, cb = table
    x = x[:n]
    pq = ProductQuantizer(16, 4, backend=cpu_be)
    pq.set_centroids(cb)
    assert pq.is_trained and np.array_equal(bits(pq.centroids), bits(cb))
    cr, dr, bad = pq_encode_ref(oracle, x, cb)
    assert not bad
    codes = pq.compute_codes(x)
    assert isinstance(codes, np.ndarray) and codes.dtype == np.uint8 and codes.shape == (n, 4)
    assert np.array_equal(codes, cr)
    codes2, dist = pq.compute_codes(x, return_distances=True)
    assert np.array_equal(codes2, cr) and dist.dtype == np.float32 and np.array_equal(bits(dist), bits(dr))
    if n >= 20:
        assert np.all(codes[10:20, 1] == 3) and np.all(dist[10:20, 1] == 0)      # not 200, the duplicate
    out = pq.decode(codes)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (n, 16)
    assert np.array_equal(bits(out), bits(pq_decode_ref(cr, cb)))
    for i in range(min(n, 5)):
        for m in range(4):
            assert np.array_equal(bits(out[i, 4 * m:4 * m + 4]), bits(cb[m, cr[i, m]]))
    t = pq.decode(torch.from_numpy(codes))                                          # a host tensor is host input
    assert np.array_equal(bits(np.asarray(t)), bits(out))


def test_constructor_and_untrained_errors(cpu_be):
    from audio_tokens_amd.ops import ProductQuantizer
    with pytest.raises(ValueError):
        ProductQuantizer(16, 3, backend=cpu_be)
    for nbits in (4, 7, 12, 16):
        with pytest.raises(NotImplementedError):
            ProductQuantizer(16, 4, nbits=nbits, backend=cpu_be)
    pq = ProductQuantizer(16, 4, backend=cpu_be)
    with pytest.raises(RuntimeError, match="not trained"):
        pq.compute_codes(np.zeros((30, 16), np.float32))
    with pytest.raises(RuntimeError, match="not trained"):
        pq.decode(np.zeros((30, 4), np.uint8))
    with pytest.raises(ValueError):
        pq.set_centroids(np.zeros((4, 128, 4), np.float32))
    with pytest.raises(ValueError):
        pq.set_centroids(np.zeros((2, 256, 8), np.float32))


@pytest.mark.parametrize("n", [40, 5])
def test_non_finite_input(cpu_be, oracle, table, n):
    from audio_tokens_amd.ops import ProductQuantizer
    x, cb = table
    x = x[:n].copy()
    x[2, 5] = np.nan
    x[3, 12] = np.inf
    x[4, 0] = -np.inf
    pq = ProductQuantizer(16, 4, backend=cpu_be)
    pq.set_centroids(cb)
    with pytest.raises(RuntimeError, match="input contains NaN's or Inf's"):
        pq.compute_codes(x)
    cr, dr, bad = pq_encode_ref(oracle, x, cb)
    assert bad and cr[2, 1] == 0 and cr[3, 3] == 0 and cr[4, 0] == 0 and np.isposinf(dr[2, 1])
    codes, dist = pq.compute_codes(x, return_distances=True, check_finite=False)
    assert np.array_equal(codes, cr) and np.array_equal(bits(dist), bits(dr))
    clean, _, _ = pq_encode_ref(oracle, table[0][:n], cb)                           # the other sub-spaces are untouched
    keep = np.ones((n, 4), bool)
    keep[2, 1] = keep[3, 3] = keep[4, 0] = False
    assert np.array_equal(codes[keep], clean[keep])


def test_float64_and_strided_input(cpu_be, oracle, table):
    from audio_tokens_amd.ops import ProductQuantizer
    x, cb = table
    pq = ProductQuantizer(16, 4, backend=cpu_be)
    pq.set_centroids(cb.astype(np.float64))
    cr, dr, _ = pq_encode_ref(oracle, x, cb)
    assert np.array_equal(pq.compute_codes(x.astype(np.float64)), cr)
    wide = np.zeros((1000, 32), np.float32)
    wide[:, ::2] = x
    codes, dist = pq.compute_codes(wide[:, ::2], return_distances=True)
    assert np.array_equal(codes, cr) and np.array_equal(bits(dist), bits(dr))
    tall = torch.zeros((2000, 16))
    tall[::2] = torch.from_numpy(x)
    assert np.array_equal(pq.compute_codes(tall[::2]), cr)
    two = np.zeros((1000, 8), np.uint8)
    two[:, ::2] = cr
    assert np.array_equal(bits(pq.decode(two[:, ::2])), bits(pq_decode_ref(cr, cb)))
    # training reads the same rows from a strided or a float64 view
    a = ProductQuantizer(16, 4, niter=2, max_points_per_centroid=2, backend=cpu_be)
    a.train(x)
    for view in (wide[:, ::2], x.astype(np.float64)):
        b = ProductQuantizer(16, 4, niter=2, max_points_per_centroid=2, backend=cpu_be)
        b.train(view)
        assert np.array_equal(bits(a.centroids), bits(b.centroids))
