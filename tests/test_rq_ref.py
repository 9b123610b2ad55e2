"""Host logic of audio_tokens_amd.ops.ResidualQuantizer driven with the CPU stand-in backend (one assign per stage and a
torch subtraction, decode by indexing and adding), against the oracle and tests/rq_ref.py: no GPU involved."""
import numpy as np
import pytest
import torch

from rq_ref import rq_decode_ref, rq_encode_ref


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture()
def cpu_be():
    from oracle_backend import OracleBackend
    return OracleBackend()


@pytest.fixture(scope="module")
def table():
    """x [1000, 16] and random codebooks for M = 3 whose later stages are finer."""
    rng = np.random.default_rng(6)
    x = rng.standard_normal((1000, 16)).astype(np.float32)
    cb = rng.standard_normal((3, 256, 16)).astype(np.float32)
    cb[1] *= np.float32(0.5)
    cb[2] *= np.float32(0.25)
    cb[:, 200] = cb[:, 3]                                  # duplicate words: the lower index wins
    x[10:20] = cb[0, 3]                                    # on a stage-0 word: zero residual into stage 1
    x[20:30] = cb[0, 7] + cb[1, 9]                         # (fp32 sum: the stage-0 answer need not be word 7)
    return x, cb


def _straight_line_training(oracle, x, M, niter, rows=None):
    """k-means on the residuals (of the rows `rows` if given), every stage advanced over ALL rows."""
    r = np.ascontiguousarray(x, dtype=np.float32)
    books = []
    for _ in range(M):
        cent = oracle.kmeans_train(r if rows is None else r[rows], 256, niter=niter).centroids
        books.append(cent)
        ids, _ = oracle.assign(r, cent)
        assert (ids >= 0).all()
        r = r - cent[ids]
    return np.stack(books, 0)


def test_exported():
    from audio_tokens_amd import ops
    assert "ResidualQuantizer" in ops.__all__


def test_train_is_one_kmeans_per_stage_on_the_residuals(cpu_be, oracle, table):
    from audio_tokens_amd.ops import Kmeans, ResidualQuantizer
    x, _ = table
    rq = ResidualQuantizer(16, 3, niter=6, backend=cpu_be)
    assert (rq.d, rq.M, rq.nbits, rq.ksub, rq.code_size) == (16, 3, 8, 256, 3)
    assert not rq.is_trained and rq.centroids is None
    rq.train(x)                                            # (n < 39 * 256: Kmeans's warning goes to stderr)
    assert rq.is_trained and rq.centroids.shape == (3, 256, 16) and rq.centroids.dtype == np.float32
    assert tuple(rq.centroids_device.shape) == (3, 256, 16)
    want = _straight_line_training(oracle, x, 3, 6)
    assert np.array_equal(bits(rq.centroids), bits(want))
    km = Kmeans(16, 256, niter=6, seed=1234, backend=cpu_be)                       # stage 0 is the plain vocabulary
    km.train(x)
    assert np.array_equal(bits(rq.centroids[0]), bits(km.centroids))
    # later stages are finer: the residual shrinks
    _, dist = rq.compute_codes(x, return_distances=True)
    assert dist[:, 2].sum() < dist[:, 1].sum() < dist[:, 0].sum()


def test_train_subsamples_every_stage_with_the_same_permutation(cpu_be, oracle, table):
    from audio_tokens_amd.ops import ResidualQuantizer
    x, _ = table
    rq = ResidualQuantizer(16, 3, niter=4, max_points_per_centroid=2, backend=cpu_be)
    rq.train(x)
    perm = cpu_be.rand_perm_prefix(1000, 1234, 512)        # faiss: rand_perm(n, seed)[:k * max_points_per_centroid]
    assert len(np.unique(perm)) == 512
    want = _straight_line_training(oracle, x, 3, 4, rows=perm)
    assert np.array_equal(bits(rq.centroids), bits(want))


def test_train_passes_kmeans_errors_and_warning_through(cpu_be, capsys):
    from audio_tokens_amd.ops import ResidualQuantizer
    rng = np.random.default_rng(1)
    rq = ResidualQuantizer(8, 2, niter=2, backend=cpu_be)
    with pytest.raises(RuntimeError, match="should be at least as large as number of clusters"):
        rq.train(rng.standard_normal((100, 8)).astype(np.float32))
    x = rng.standard_normal((300, 8)).astype(np.float32)
    x[7, 5] = np.nan
    with pytest.raises(RuntimeError, match="NaN's or Inf's"):
        rq.train(x)
    assert not rq.is_trained
    x[7, 5] = 0.0
    capsys.readouterr()
    rq.train(x)
    assert capsys.readouterr().err.count("WARNING clustering 300 points to 256 centroids") == 2
    assert rq.is_trained


@pytest.mark.parametrize("n", [300, 12, 0])
def test_encode_and_decode_against_the_reference(cpu_be, oracle, table, n):
    from audio_tokens_amd.ops import ResidualQuantizer
    x, cb = table
    x = x[:n]
    rq = ResidualQuantizer(16, 3, backend=cpu_be)
    rq.set_centroids(cb)
    assert rq.is_trained and np.array_equal(bits(rq.centroids), bits(cb))
    cr, dr, rr, bad = rq_encode_ref(oracle, x, cb)
    assert not bad
    codes = rq.compute_codes(x)
    assert isinstance(codes, np.ndarray) and codes.dtype == np.uint8 and codes.shape == (n, 3)
    assert np.array_equal(codes, cr)
    codes2, dist, res = rq.compute_codes(x, return_distances=True, return_residual=True)
    assert np.array_equal(codes2, cr) and dist.dtype == np.float32 and np.array_equal(bits(dist), bits(dr))
    assert res.dtype == np.float32 and res.shape == (n, 16) and np.array_equal(bits(res), bits(rr))
    codes3, res3 = rq.compute_codes(x, return_residual=True)                        # the tuple keeps its order
    assert np.array_equal(codes3, cr) and np.array_equal(bits(res3), bits(rr))
    if n:
        # a row on a stage-0 word: distance 0, the first copy of the word, an exactly zero residual into stage 1
        assert np.all(codes[10:12, 0] == 3) and np.all(dist[10:12, 0] == 0)
        one = ResidualQuantizer(16, 1, backend=cpu_be)
        one.set_centroids(cb[:1])
        c1, r1 = one.compute_codes(x, return_residual=True)
        assert np.array_equal(c1[:, 0], cr[:, 0]) and np.all(r1[10:12] == 0)
        # the defined sums (decode + residual == x is not one of them: fp32 addition does not invert the subtractions)
        r = x.copy()
        for m in range(3):
            r = r - cb[m][cr[:, m]]
        assert np.array_equal(bits(r), bits(rr))
    out = rq.decode(codes)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (n, 16)
    assert np.array_equal(bits(out), bits(rq_decode_ref(cr, cb)))
    if n:
        want = (cb[0][cr[:, 0]] + cb[1][cr[:, 1]]) + cb[2][cr[:, 2]]
        assert np.array_equal(bits(out), bits(want))
    t = rq.decode(torch.from_numpy(codes))                                          # a host tensor is host input
    assert np.array_equal(bits(np.asarray(t)), bits(out))
    # any prefix of the code is the code of the shorter quantiser
    two = ResidualQuantizer(16, 2, backend=cpu_be)
    two.set_centroids(cb[:2])
    assert np.array_equal(two.compute_codes(x), cr[:, :2])


def test_constructor_and_untrained_errors(cpu_be):
    from audio_tokens_amd.ops import ResidualQuantizer
    for d, M in ((0, 2), (16, 0), (-4, 1)):
        with pytest.raises(ValueError):
            ResidualQuantizer(d, M, backend=cpu_be)
    for nbits in (4, 7, 12, 16):
        with pytest.raises(NotImplementedError):
            ResidualQuantizer(16, 4, nbits=nbits, backend=cpu_be)
    for beam in (0, 2, 5):
        with pytest.raises(NotImplementedError):
            ResidualQuantizer(16, 4, max_beam_size=beam, backend=cpu_be)
    rq = ResidualQuantizer(16, 3, backend=cpu_be)                                   # d need not be a multiple of M
    with pytest.raises(RuntimeError, match="not trained"):
        rq.compute_codes(np.zeros((30, 16), np.float32))
    with pytest.raises(RuntimeError, match="not trained"):
        rq.decode(np.zeros((30, 3), np.uint8))
    with pytest.raises(ValueError):
        rq.set_centroids(np.zeros((3, 128, 16), np.float32))
    with pytest.raises(ValueError):
        rq.set_centroids(np.zeros((2, 256, 16), np.float32))
    with pytest.raises(ValueError):
        rq.set_centroids(np.zeros((3, 256, 8), np.float32))
    rq.set_centroids(np.zeros((3, 256, 16), np.float32))
    with pytest.raises(AssertionError):
        rq.compute_codes(np.zeros((30, 8), np.float32))
    with pytest.raises(AssertionError):
        rq.decode(np.zeros((30, 2), np.uint8))
    with pytest.raises(AssertionError):
        rq.decode(np.zeros((30, 3), np.int64))


@pytest.mark.parametrize("n", [40, 5])
def test_non_finite_input(cpu_be, oracle, table, n):
    from audio_tokens_amd.ops import ResidualQuantizer
    x, cb = table
    x = x[:n].copy()
    x[2, 5] = np.nan
    x[3, 12] = np.inf
    x[4, :] = 3e19                                        # |x|^2 overflows
    rq = ResidualQuantizer(16, 3, backend=cpu_be)
    rq.set_centroids(cb)
    with pytest.raises(RuntimeError, match="input contains NaN's or Inf's"):
        rq.compute_codes(x)
    cr, dr, rr, bad = rq_encode_ref(oracle, x, cb)
    assert bad and np.all(cr[2:5] == 0) and np.all(np.isposinf(dr[2:5]))            # at every stage
    codes, dist, res = rq.compute_codes(x, return_distances=True, return_residual=True, check_finite=False)
    assert np.array_equal(codes, cr) and np.array_equal(bits(dist), bits(dr)) and np.array_equal(bits(res), bits(rr))
    assert np.isnan(res[2, 5]) and np.isposinf(res[3, 12])                          # a flagged row subtracts word 0
    want = ((x[2] - cb[0, 0]) - cb[1, 0]) - cb[2, 0]
    assert np.array_equal(bits(res[2])[np.arange(16) != 5], bits(want)[np.arange(16) != 5])
    clean = rq_encode_ref(oracle, table[0][:n], cb)                                 # the other rows are untouched
    keep = np.ones(n, bool)
    keep[2:5] = False
    assert np.array_equal(codes[keep], clean[0][keep]) and np.array_equal(bits(res[keep]), bits(clean[2][keep]))


def test_float64_and_strided_input(cpu_be, oracle, table):
    from audio_tokens_amd.ops import ResidualQuantizer
    x, cb = table
    x = x[:300]
    rq = ResidualQuantizer(16, 3, backend=cpu_be)
    rq.set_centroids(cb.astype(np.float64))
    cr, dr, rr, _ = rq_encode_ref(oracle, x, cb)
    assert np.array_equal(rq.compute_codes(x.astype(np.float64)), cr)
    wide = np.zeros((300, 32), np.float32)
    wide[:, ::2] = x
    codes, dist, res = rq.compute_codes(wide[:, ::2], return_distances=True, return_residual=True)
    assert np.array_equal(codes, cr) and np.array_equal(bits(dist), bits(dr)) and np.array_equal(bits(res), bits(rr))
    tall = torch.zeros((600, 16))
    tall[::2] = torch.from_numpy(x)
    assert np.array_equal(rq.compute_codes(tall[::2]), cr)
    two = np.zeros((300, 6), np.uint8)
    two[:, ::2] = cr
    assert np.array_equal(bits(rq.decode(two[:, ::2])), bits(rq_decode_ref(cr, cb)))
    # training reads the same rows from a strided or a float64 view
    a = ResidualQuantizer(16, 2, niter=2, max_points_per_centroid=1, backend=cpu_be)
    a.train(x)
    for view in (wide[:, ::2], x.astype(np.float64)):
        b = ResidualQuantizer(16, 2, niter=2, max_points_per_centroid=1, backend=cpu_be)
        b.train(view)
        assert np.array_equal(bits(a.centroids), bits(b.centroids))
