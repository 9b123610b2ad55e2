"""The CPU reference of spherical k-means (tests/spherical_ref.py) held to glibc's fmaf and to independent code, and
the host logic of ops.Kmeans(spherical=True) / ops.IndexFlatIP driven with the reference's backend: no GPU involved."""
import ctypes
import ctypes.util
import os
import socket
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

from spherical_ref import (SphericalOracleBackend, fma32, fma32_naive, ip_matrix, renorm_ref, search_ip_ref,
                           spherical_kmeans_ref)

G = Path(__file__).resolve().parent / "golden"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _tie_family(rng, m, sign):
    """a * b = ulp(c) / 2 * (1 - 2^-46): fmaf(sign * a, b, c) lies just inside the half-ulp on either side of c (the
    correct result is c), and a float64 multiply-add lands exactly on the tie."""
    c = (rng.uniform(1.0, 2.0, m) * 2.0 ** rng.integers(-20, 20, m)).astype(np.float32)
    a = (np.spacing(c).astype(np.float64) / 2 * (1 + 2.0 ** -23)).astype(np.float32)
    b = np.full(m, 1 - 2.0 ** -23, np.float32)
    return (sign * a).astype(np.float32), b, c


@pytest.fixture(scope="module")
def spherical_be():
    return SphericalOracleBackend()


# ---- 1. fma32 is fmaf -----------------------------------------------------------------------------
def test_fma32_equals_libm_fmaf_bit_for_bit():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(11)
    parts = []
    m = 30000
    parts.append(tuple(rng.standard_normal(m).astype(np.float32) for _ in range(3)))
    parts.append(tuple((rng.standard_normal(m) * 10.0 ** rng.integers(-30, 30, m)).astype(np.float32) for _ in range(3)))
    parts.append(tuple(rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32).view(np.float32) for _ in range(3)))
    a, b, _ = parts[0]                                           # heavy cancellation: c = -round(a * b)
    parts.append((a, b, (-(a * b)).astype(np.float32)))
    below, above = _tie_family(rng, m, 1.0), _tie_family(rng, m, -1.0)
    parts += [below, above]
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3e38, -3e38, 1e-25], np.float32)
    sa, sb, sc = np.meshgrid(special, special, special, indexing="ij")
    parts.append((sa.ravel(), sb.ravel(), sc.ravel()))
    a, b, c = (np.concatenate([p[i] for p in parts]) for i in range(3))
    assert a.size >= 100000
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = fma32(a, b, c)
    want = np.array([libm.fmaf(float(u), float(v), float(w)) for u, v, w in zip(a, b, c)], np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])
    # the shortcut rounds twice: on both tie families it is wrong about half of the time, fma32 never
    for fa, fb, fc in (below, above):
        exact = fma32(fa, fb, fc)
        assert np.array_equal(bits(exact), bits(fc))
        wrong = (bits(fma32_naive(fa, fb, fc)) != bits(exact)).mean()
        assert 0.25 < wrong < 0.75, wrong


# ---- 2. against independent code ------------------------------------------------------------------
def test_search_ip_names_the_oracles_nearest_centroid(oracle):
    rng = np.random.default_rng(5)
    c = rng.standard_normal((64, 64)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    label = rng.integers(0, 64, 1500)
    x = c[label] + np.float32(0.01) * rng.standard_normal((1500, 64)).astype(np.float32)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    ids, best = search_ip_ref(x, c)
    top2 = np.sort(ip_matrix(x, c).astype(np.float64), axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-5
    assert clear.mean() >= 0.99
    ids_l2, _ = oracle.assign(x, c)
    assert np.array_equal(ids[clear], ids_l2[clear])
    assert np.array_equal(ids[clear], label[clear])
    assert np.array_equal(bits(best), bits(ip_matrix(x, c)[np.arange(1500), ids]))


def test_search_ip_listing_rule():
    x = np.array([[1, 2], [np.nan, 1], [0, 0], [np.inf, 1], [-1, -1]], np.float32)
    c = np.array([[-1, -1], [np.nan, 0], [2, 1], [2, 1], [0, 0]], np.float32)
    ids, best = search_ip_ref(x, c)
    assert list(ids) == [2, -1, 0, 2, 0]
    assert np.array_equal(bits(best), bits(np.array([4, -np.inf, 0, np.inf, 2], np.float32)))


def test_renorm_ref_rows():
    c = np.array([[3, 4], [0, 0], [1e-25, 1e-25], [1e20, 1e20], [np.nan, 1]], np.float32)
    out = renorm_ref(c)
    assert np.array_equal(bits(out[0]), bits(np.array([3, 4], np.float32) * (np.float32(1) / np.float32(5))))
    assert np.array_equal(bits(out[1:3]), bits(c[1:3]))           # zero norm (the squares underflow): untouched
    assert np.array_equal(out[3], [0, 0])                         # the norm overflows: inv = 0
    assert np.array_equal(bits(out[4]), bits(c[4]))


# ---- 3. host logic of ops.Kmeans(spherical=True) == the straight-line loop ------------------------------
def _same(km, r):
    assert np.array_equal(bits(km.centroids), bits(r.centroids))
    assert [s["nsplit"] for s in km.iteration_stats] == r.nsplit
    np.testing.assert_allclose(km.obj, np.array(r.obj, np.float32), rtol=2e-6)


def test_cold_and_warm_start_match_the_loop(spherical_be, oracle):
    from audio_tokens_amd.ops import IndexFlatIP, Kmeans
    g = np.load(G / "kmeans.npz")
    km = Kmeans(64, 64, niter=5, spherical=True, backend=spherical_be)
    obj = km.train(g["a_x"])
    r1 = spherical_kmeans_ref(g["a_x"], 64, 5)
    _same(km, r1)
    assert obj == pytest.approx(r1.obj[-1], rel=2e-6)
    assert isinstance(km.index, IndexFlatIP) and km.index.ntotal == 64
    # every centroid is a unit row, and without a split the objective does not decrease
    nrm = np.linalg.norm(km.centroids.astype(np.float64), axis=1)
    assert np.abs(nrm - 1).max() < 1e-6
    for i in range(1, 5):
        if r1.nsplit[i - 1] == 0:
            assert r1.obj[i] >= r1.obj[i - 1] * (1 - 2e-6)
    D, I = km.index.search(g["a_x"][:50], 1)
    ids, best = search_ip_ref(g["a_x"][:50], r1.centroids)
    assert D.shape == (50, 1) and I.dtype == np.int64 and D.dtype == np.float32
    assert np.array_equal(I[:, 0], ids) and np.array_equal(bits(D[:, 0]), bits(best))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km.train(g["b_x"], init_centroids=km.centroids)   # the reference's loop: the next batch, warm
    r2 = spherical_kmeans_ref(g["b_x"], 64, 5, init=r1.centroids)
    _same(km, r2)


def test_subsampled_run_matches_the_loop(spherical_be, oracle):
    from audio_tokens_amd.ops import Kmeans
    x = np.load(G / "kmeans.npz")["c_x"]
    assert x.shape[0] > 256 * 64
    km = Kmeans(8, 64, niter=3, spherical=True, backend=spherical_be)
    km.train(x)
    _same(km, spherical_kmeans_ref(x, 64, 3))


def test_duplicate_initial_centroids_split_in_iteration_0(spherical_be, oracle):
    """Two identical rows in init_centroids: ties go to the lowest index, the higher copy receives no point, and
    split_clusters fires in iteration 0 by construction."""
    from audio_tokens_amd.ops import Kmeans
    x = np.load(G / "kmeans.npz")["a_x"][:1500]
    init = x[np.arange(48) * 31].copy()
    init[29] = init[7]
    km = Kmeans(64, 48, niter=4, spherical=True, backend=spherical_be)
    km.train(x, init_centroids=init)
    r = spherical_kmeans_ref(x, 48, 4, init=init)
    assert r.nsplit[0] >= 1
    _same(km, r)
    assert np.abs(np.linalg.norm(km.centroids.astype(np.float64), axis=1) - 1).max() < 1e-6


# ---- 4. / 5. corner cases and the constructor ----------------------------------------------------------
def test_ns_equal_k_returns_the_rows_unnormalised(spherical_be):
    from audio_tokens_amd.ops import IndexFlatIP, Kmeans
    x = (np.random.default_rng(0).standard_normal((10, 4)) * 3).astype(np.float32)
    km = Kmeans(4, 10, niter=3, spherical=True, backend=spherical_be)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km.train(x)
    assert np.array_equal(bits(km.centroids), bits(x)) and km.iteration_stats[0]["nsplit"] == 0
    assert np.array_equal(bits(spherical_kmeans_ref(x, 10, 3).centroids), bits(x))
    assert isinstance(km.index, IndexFlatIP) and km.index.ntotal == 10


def test_constructor_rules(spherical_be):
    from oracle_backend import OracleBackend
    from audio_tokens_amd.ops import Kmeans
    with pytest.raises(NotImplementedError):
        Kmeans(4, 2, spherical=True, backend=OracleBackend())
    assert Kmeans(4, 2, spherical=True, backend=spherical_be).spherical
    assert not Kmeans(4, 2, backend=spherical_be).spherical
    for bad in (dict(nredo=2), dict(int_centroids=True), dict(frozen_centroids=True)):
        with pytest.raises(NotImplementedError):
            Kmeans(4, 2, spherical=True, backend=spherical_be, **bad)
    x = np.random.default_rng(0).standard_normal((10, 4)).astype(np.float32)
    with pytest.raises(RuntimeError, match="should be at least as large as number of clusters"):
        Kmeans(4, 16, spherical=True, backend=spherical_be).train(x)
    x[2, 1] = np.inf
    with pytest.raises(RuntimeError, match="NaN's or Inf's"):
        Kmeans(4, 4, spherical=True, backend=spherical_be).train(x)


def test_index_flat_ip_host_rules(spherical_be):
    from audio_tokens_amd import ops
    assert "IndexFlatIP" in ops.__all__
    rng = np.random.default_rng(2)
    c, x = rng.standard_normal((30, 12)).astype(np.float32), rng.standard_normal((40, 12)).astype(np.float32)
    index = ops.IndexFlatIP(12, backend=spherical_be)
    assert index.ntotal == 0
    D, I = index.search(x, 1)
    assert D.shape == (40, 1) and (D == -np.inf).all() and (I == -1).all() and I.dtype == np.int64
    index.add(c[:10]); index.add(c[10:])
    assert index.ntotal == 30
    D, I = index.search(x)
    ids, best = search_ip_ref(x, c)
    assert np.array_equal(I[:, 0], ids) and np.array_equal(bits(D[:, 0]), bits(best))
    with pytest.raises(RuntimeError):
        index.search(x, 0)
    with pytest.raises(NotImplementedError):
        index.search(x, 2)
    index.reset()
    assert index.ntotal == 0


# ---- 6. world_size 2 under gloo ----------------------------------------------------------------
def _exact_sum_rows():
    """Rows whose entries are multiples of 2^-8 below 4 in magnitude: every fp32 sum of fewer than 2^13 of them is
    exact, so the order in which two shards' partial sums are added cannot show and the sharded run has to give the
    single-process bits.  (Spherical k-means does not need unit rows.)"""
    x = np.load(G / "kmeans.npz")["a_x"]
    return (np.round(x * 8 * 256) / 256).astype(np.float32)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from audio_tokens_amd.ops import Kmeans
        x, cut = _exact_sum_rows(), 900
        local = x[:cut] if rank == 0 else x[cut:]
        km = Kmeans(64, 64, niter=5, spherical=True, distributed=True, backend=SphericalOracleBackend())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            km.train(local)
        q.put((rank, km.centroids.copy(), [s["nsplit"] for s in km.iteration_stats], km.obj.copy()))
    finally:
        dist.destroy_process_group()


def test_sharded_spherical_kmeans_gloo_world2(spherical_be, oracle):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    from audio_tokens_amd.ops import Kmeans
    x = _exact_sum_rows()
    km = Kmeans(64, 64, niter=5, spherical=True, backend=spherical_be)
    km.train(x)
    r = spherical_kmeans_ref(x, 64, 5)
    _same(km, r)
    for rank, cent, nsplit, obj in res:
        assert np.array_equal(bits(cent), bits(km.centroids)), f"rank {rank} differs from the single-process run"
        assert nsplit == r.nsplit
        np.testing.assert_allclose(obj, km.obj, rtol=2e-6)
