"""at_assign_ip_f32, at_renorm_rows_f32, ops.IndexFlatIP and ops.Kmeans(spherical=True) on the device against the
numpy reference of tests/spherical_ref.py: ids equal, products and centroids bit for bit."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from audio_tokens_amd import _lib
from spherical_ref import ip_matrix, renorm_ref, search_ip_ref, spherical_kmeans_ref

pytestmark = pytest.mark.gpu

# the smallest shapes at which each thing can still go wrong: one and several 128-centroid tiles with a partial last
# tile, row tails inside a wave and a workgroup, both register-resident widths, one-chunk and multi-chunk widths with a
# partial last chunk, and the scalar form
GRID = [(64, 1, 1), (64, 5, 19), (64, 33, 33), (64, 129, 257), (64, 300, 1000),
        (128, 130, 300), (128, 600, 200),
        (8, 7, 100), (32, 40, 70), (200, 70, 65), (640, 33, 40),
        (6, 10, 50), (7, 3, 21),
        # a second workgroup with one live row and a second tile with one real centroid at every form of the sweep;
        # a second chunk of one 16-byte piece (d = 68), three chunks (d = 192)
        (64, 129, 129), (128, 129, 129), (68, 129, 129), (192, 129, 129)]
FAMILY_SHAPES = [(64, 129, 257), (128, 130, 300), (200, 70, 65)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _near_centroids(rng, d, k, n):
    c = _unit(rng.standard_normal((k, d)))
    x = _unit(c[rng.integers(0, k, n)] + 0.05 * rng.standard_normal((n, d)))
    return x, c


def _check(be, x, c):
    """be.assign_ip against the reference -> (ids, ip) of the reference."""
    ids, ip = be.assign_ip(be.from_host(x), be.from_host(c))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ids_r, ip_r = search_ip_ref(x, c)
    got_i, got_v = ids.cpu().numpy(), ip.cpu().numpy()
    assert got_i.dtype == np.int64 and got_v.dtype == np.float32
    bad = np.nonzero(got_i != ids_r)[0]
    assert bad.size == 0, (bad[:5], got_i[bad[:5]], ids_r[bad[:5]])
    assert np.array_equal(bits(got_v), bits(ip_r))
    return ids_r, ip_r


@pytest.mark.parametrize("d,k,n", GRID)
def test_sweep_grid(be, d, k, n):
    x, c = _near_centroids(np.random.default_rng(d * 1000 + k), d, k, n)
    _check(be, x, c)


@pytest.mark.parametrize("d,k,n", FAMILY_SHAPES)
def test_padding_never_wins_when_every_product_is_negative(be, d, k, n):
    rng = np.random.default_rng(k)
    x = rng.uniform(0.1, 1.0, (n, d)).astype(np.float32)
    c = -rng.uniform(0.1, 1.0, (k, d)).astype(np.float32)
    ids, ip = _check(be, x, c)
    assert (ip < 0).all() and (ids >= 0).all() and (ids < k).all()


@pytest.mark.parametrize("d,k,n", FAMILY_SHAPES)
def test_duplicate_centroids_lowest_index_wins(be, d, k, n):
    """Identical centroid rows give identical chains.  j + 16 sits in another register of the same lane, j + 32 in
    its next accumulator, j + 4 in the other half-wave and j + 128 in the next tile."""
    rng = np.random.default_rng(k + 1)
    x, c = _near_centroids(rng, d, k, n)
    groups = []
    for j in (0, 1, 9):
        copies = [j + o for o in (4, 16, 32, 128) if j + o < k]
        c[copies] = c[j]
        groups.append((j, copies))
    # rows on the copies themselves, and on every subset that lacks its lowest members
    x[:3] = c[[0, 1, 9]]
    ids, _ = _check(be, x, c)
    assert list(ids[:3]) == [0, 1, 9]
    for j, copies in groups:                # the original moved away: the lowest remaining copy has to win
        c2 = c.copy()
        for drop in [j] + copies[:-1]:
            c2[drop] = -c[j]
            ids2, _ = _check(be, x[:40], c2)
            rest = [q for q in [j] + copies if not np.array_equal(c2[q], -c[j])]
            row = [0, 1, 9].index(j)
            assert ids2[row] == min(rest)


@pytest.mark.parametrize("d,k,n", FAMILY_SHAPES)
def test_zero_row_and_zero_centroid(be, d, k, n):
    rng = np.random.default_rng(k + 2)
    x, c = _near_centroids(rng, d, k, n)
    x[3] = 0
    ids, ip = _check(be, x, c)
    assert ids[3] == 0 and bits(ip[3:4])[0] == 0                  # +0.0, the lowest index
    x = rng.uniform(0.1, 1.0, (n, d)).astype(np.float32)
    c = -rng.uniform(0.1, 1.0, (k, d)).astype(np.float32)
    c[k // 2] = 0
    ids, ip = _check(be, x, c)
    assert (ids == k // 2).all() and (bits(ip) == 0).all()


@pytest.mark.parametrize("d,k,n", FAMILY_SHAPES)
def test_bad_values(be, d, k, n):
    rng = np.random.default_rng(k + 3)
    x, c = _near_centroids(rng, d, k, n)
    x[5, d // 2] = np.nan
    x[n - 1, 0] = np.nan
    ids, ip = _check(be, x, c)
    assert ids[5] == -1 and ids[n - 1] == -1 and ip[5] == -np.inf and ip[n - 1] == -np.inf
    x, c = _near_centroids(rng, d, k, n)
    c[x[:20].astype(np.float64).dot(c.T.astype(np.float64)).argmax(axis=1), 1] = np.nan   # the winners of 20 rows
    c[k - 1] = np.nan
    ids, ip = _check(be, x, c)
    assert not np.isnan(c[ids]).any() and np.isfinite(ip).all()
    x, c = _near_centroids(rng, d, k, n)
    x[7, 2] = np.inf                                              # +inf / -inf / NaN (0 * inf) products by the sign of c[:, 2]
    x[8, d - 1] = -np.inf
    c[4, 2] = 0
    ids, ip = _check(be, x, c)
    assert ip[7] == np.inf and ip[8] == np.inf


def test_rows_off_a_16_byte_boundary_give_the_aligned_bits(be):
    x, c = _near_centroids(np.random.default_rng(8), 64, 129, 257)
    ids_r, ip_r = _check(be, x, c)
    buf = be.empty((257 * 64 + 4,))
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + 257 * 64].view(257, 64)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    ids, ip = be.assign_ip(view, be.from_host(c))
    assert np.array_equal(ids.cpu().numpy(), ids_r) and np.array_equal(bits(ip.cpu().numpy()), bits(ip_r))


def test_assign_ip_two_streams_at_once(be):
    """Two calls with different centroid tables on two streams of one backend share the context's centroid image
    (WS_IP_IMG): the later one waits for the earlier one, and both give the single-stream bits.  This cannot prove the
    absence of a race; it pins the guarded path, and runs in milliseconds."""
    rng = np.random.default_rng(77)
    x1, c1 = _near_centroids(rng, 64, 300, 4096)
    x2, c2 = _near_centroids(rng, 64, 170, 4100)
    t = [be.from_host(a) for a in (x1, c1, x2, c2)]
    want = [be.assign_ip(t[0], t[1]), be.assign_ip(t[2], t[3])]
    torch.cuda.synchronize(be.device)
    s1, s2 = torch.cuda.Stream(be.device), torch.cuda.Stream(be.device)
    s1.wait_stream(torch.cuda.current_stream(be.device))
    s2.wait_stream(torch.cuda.current_stream(be.device))
    with torch.cuda.stream(s1):
        r1 = be.assign_ip(t[0], t[1])
    with torch.cuda.stream(s2):
        r2 = be.assign_ip(t[2], t[3])
    with torch.cuda.stream(s1):
        r3 = be.assign_ip(t[0], t[1])
    torch.cuda.synchronize(be.device)
    for got, ref in zip((r1, r2, r3), (want[0], want[1], want[0])):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))


def test_want_dist_false(be):
    x, c = _near_centroids(np.random.default_rng(9), 64, 129, 257)
    xt, ct = be.from_host(x), be.from_host(c)
    ids, ip = be.assign_ip(xt, ct)
    ids2, none = be.assign_ip(xt, ct, want_dist=False)
    assert none is None and torch.equal(ids, ids2)


def test_index_flat_ip_search(be):
    from audio_tokens_amd.ops import IndexFlatIP
    x, c = _near_centroids(np.random.default_rng(10), 64, 129, 257)
    index = IndexFlatIP(64, backend=be)
    D, I = index.search(x, 1)                                     # empty index
    assert isinstance(D, np.ndarray) and D.shape == (257, 1) and (D == -np.inf).all() and (I == -1).all()
    index.add(c[:100]); index.add(be.from_host(c[100:]))
    assert index.ntotal == 129
    D, I = index.search(x, 1)
    assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray) and D.shape == I.shape == (257, 1)
    assert D.dtype == np.float32 and I.dtype == np.int64
    ids_r, ip_r = search_ip_ref(x, c)
    assert np.array_equal(I[:, 0], ids_r) and np.array_equal(bits(D[:, 0]), bits(ip_r))
    Dt, It = index.search(be.from_host(x))
    assert isinstance(Dt, torch.Tensor) and Dt.device == be.device and It.device == be.device
    assert np.array_equal(It.cpu().numpy(), I) and np.array_equal(bits(Dt.cpu().numpy()), bits(D))
    ids, ip = index.assign(be.from_host(x), want_dist=False)
    assert ip is None and np.array_equal(ids.cpu().numpy(), ids_r)
    with pytest.raises(RuntimeError):
        index.search(x, 0)
    with pytest.raises(NotImplementedError):
        index.search(x, 2)
    D0, I0 = index.search(np.zeros((0, 64), np.float32), 1)
    assert D0.shape == (0, 1) and I0.shape == (0, 1)
    index.reset()
    assert index.ntotal == 0


def test_abi_argument_errors(be):
    """Every bad call returns a negative code and a message before anything is launched."""
    lib, h = be.lib, be.ctx.handle
    x, c = be.zeros((32, 64)), be.zeros((8, 64))
    ids, ip = be.empty((32,), torch.int64), be.empty((32,))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = be._stream()

    def fails(rc, text):
        assert rc < 0 and text in _lib.last_error(), (rc, _lib.last_error())

    fails(lib.at_assign_ip_f32(None, p(x), 32, 64, p(c), 8, p(ids), p(ip), s), "ctx is null")
    fails(lib.at_assign_ip_f32(h, p(x), 32, 0, p(c), 8, p(ids), p(ip), s), "bad sizes")
    fails(lib.at_assign_ip_f32(h, p(x), 32, 64, p(c), 0, p(ids), p(ip), s), "bad sizes")
    fails(lib.at_assign_ip_f32(h, p(x), -1, 64, p(c), 8, p(ids), p(ip), s), "bad sizes")
    fails(lib.at_assign_ip_f32(h, p(x), 32, 64, p(c), (1 << 24) + 1, p(ids), p(ip), s), "too large")
    fails(lib.at_assign_ip_f32(h, p(x), 32, 64, p(c), 8, None, p(ip), s), "null pointer")
    fails(lib.at_assign_ip_f32(h, None, 32, 64, p(c), 8, p(ids), p(ip), s), "null pointer")
    assert lib.at_assign_ip_f32(h, None, 0, 64, None, 8, None, None, s) == 0          # n == 0: nothing to do
    fails(lib.at_renorm_rows_f32(None, p(c), 8, 64, s), "ctx is null")
    fails(lib.at_renorm_rows_f32(h, p(c), 8, 0, s), "bad sizes")
    fails(lib.at_renorm_rows_f32(h, p(c), -1, 64, s), "bad sizes")
    fails(lib.at_renorm_rows_f32(h, None, 8, 64, s), "null pointer")
    assert lib.at_renorm_rows_f32(h, None, 0, 64, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(c, torch.zeros_like(c))


@pytest.mark.parametrize("k,d", [(1, 1), (5, 6), (64, 64), (500, 128), (33, 640)])
def test_renorm_rows(be, k, d):
    rng = np.random.default_rng(k)
    c = (rng.standard_normal((k, d)) * 10.0 ** rng.integers(-3, 4, (k, 1))).astype(np.float32)
    if k >= 5:
        c[1] = 0
        c[2] = 1e-25                                             # the squares underflow to zero: untouched
        c[3] = 1e20                                              # the norm overflows: inv = 0
        c[4, d // 2] = np.nan
    t = be.from_host(c)
    out = be.renorm_rows(t)
    assert out is t
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = renorm_ref(c)
    got = t.cpu().numpy()
    assert np.array_equal(bits(got), bits(ref))
    if k >= 5:
        assert np.array_equal(bits(got[1:3]), bits(c[1:3])) and (got[3] == 0).all() and np.array_equal(bits(got[4]), bits(c[4]))


def _same(km, r):
    assert np.array_equal(bits(km.centroids), bits(r.centroids))
    assert [s["nsplit"] for s in km.iteration_stats] == r.nsplit
    np.testing.assert_allclose(km.obj, np.array(r.obj, np.float32), rtol=2e-6)


@pytest.mark.parametrize("n,d,k,niter", [(2000, 64, 40, 8), (3000, 8, 8, 3), (1000, 128, 16, 3)])
def test_spherical_kmeans_matches_the_loop(be, oracle, n, d, k, niter):
    from audio_tokens_amd.ops import IndexFlatIP, Kmeans
    x, _ = _near_centroids(np.random.default_rng(n), d, k, n)
    km = Kmeans(d, k, niter=niter, spherical=True, backend=be)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km.train(x)
    _same(km, spherical_kmeans_ref(x, k, niter))
    assert isinstance(km.index, IndexFlatIP) and km.index.ntotal == k
    assert np.abs(np.linalg.norm(km.centroids.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_spherical_kmeans_duplicate_init_warm_start_and_index(be, oracle):
    from audio_tokens_amd.ops import Kmeans
    rng = np.random.default_rng(77)
    x, _ = _near_centroids(rng, 64, 48, 1500)
    init = x[np.arange(48) * 31].copy()
    init[29] = init[7]                                            # the higher copy receives no point: a split in iteration 0
    km = Kmeans(64, 48, niter=4, spherical=True, backend=be)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km.train(x, init_centroids=init)
        r1 = spherical_kmeans_ref(x, 48, 4, init=init)
        assert r1.nsplit[0] >= 1
        _same(km, r1)
        x2, _ = _near_centroids(rng, 64, 48, 1200)
        km.train(x2, init_centroids=km.centroids_device)
        _same(km, spherical_kmeans_ref(x2, 48, 4, init=r1.centroids))
    xt = be.from_host(x2)
    D, I = km.index.search(xt, 1)
    ids, ip = be.assign_ip(xt, km.centroids_device)
    assert torch.equal(I[:, 0], ids) and torch.equal(D[:, 0].view(torch.int32), ip.view(torch.int32))
