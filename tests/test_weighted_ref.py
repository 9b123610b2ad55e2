"""The CPU reference of weighted k-means (tests/weighted_ref.py) on hand-computed cases, and the host logic of
ops.Kmeans.train(x, weights=w) driven with the reference's backend: no GPU involved."""
import os
import socket
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle_backend import OracleBackend
from weighted_ref import (SphericalWeightedOracleBackend, WeightedOracleBackend, full_mantissa_weights, imbalance_ref,
                          weighted_kmeans_ref, weighted_sums, weighted_sums_loop, weighted_sums_two_roundings)

G = Path(__file__).resolve().parent / "golden"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def wbe():
    return WeightedOracleBackend()


@pytest.fixture(scope="module")
def golden():
    return np.load(G / "kmeans.npz")


def _train(be, x, w, k, niter, d=None, **kw):
    from audio_tokens_amd.ops import Kmeans
    ctor = {n: kw.pop(n) for n in ("spherical", "max_points_per_centroid") if n in kw}
    km = Kmeans(d or x.shape[1], k, niter=niter, backend=be, **ctor)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km.train(x, weights=w, **kw)
    return km


def _same(km, r):
    assert np.array_equal(bits(km.centroids), bits(r.centroids))
    st = km.iteration_stats
    assert [s["nsplit"] for s in st] == r.nsplit
    assert np.array_equal(bits(km.obj), bits(np.array(r.obj, np.float32)))
    assert [s["imbalance_factor"] for s in st] == r.imbalance


# ---- 1. the reference itself ------------------------------------------------------------------------------
def test_reference_on_hand_computed_cases():
    x = np.array([[1, 2], [3, 4], [5, 6], [7, 8]], np.float32)
    w = np.array([2, 0.5, 1, 3], np.float32)
    sums, wsum, order, sid = weighted_sums(x, w, np.array([0, 1, 0, 7]), 3)
    assert np.array_equal(sums, [[7, 10], [1.5, 2], [0, 0]]) and np.array_equal(wsum, [3, 0.5, 0])
    assert list(order) == [0, 2, 1, 3] and list(sid) == [0, 0, 1, 3]           # id 7 parked in bucket k = 3
    # one rounding per member: -1 + (1 + 2^-12)^2 = 2^-11 + 2^-24 exactly; the rounded product is 1 + 2^-11 (tie to even)
    a = np.float32(1 + 2.0 ** -12)
    x = np.array([[-1], [a]], np.float32)
    w = np.array([1, a], np.float32)
    sums, wsum, _, _ = weighted_sums(x, w, np.zeros(2, np.int64), 1)
    assert sums[0, 0] == np.float32(2.0 ** -11 + 2.0 ** -24) and wsum[0] == np.float32(2) + np.float32(2.0 ** -12)
    two, _, _, _ = weighted_sums_two_roundings(x, w, np.zeros(2, np.int64), 1)
    assert two[0, 0] == np.float32(2.0 ** -11)
    # the order is ascending row: (2^24 + 1) + 1 rounds twice to 2^24, 1 + 1 + 2^24 is exact
    big = np.float32(2.0 ** 24)
    up, wup, _, _ = weighted_sums(np.array([[big], [1], [1]], np.float32), np.ones(3, np.float32), np.zeros(3, np.int64), 1)
    down, _, _, _ = weighted_sums(np.array([[1], [1], [big]], np.float32), np.ones(3, np.float32), np.zeros(3, np.int64), 1)
    assert up[0, 0] == big and down[0, 0] == big + np.float32(2) and wup[0] == 3
    # zero weights: the member counts for nothing; -0 + +0 = +0
    s, ws, _, _ = weighted_sums(np.array([[5], [-3]], np.float32), np.array([0.0, -0.0], np.float32), np.zeros(2, np.int64), 2)
    assert np.array_equal(bits(s), bits(np.zeros((2, 1), np.float32))) and np.array_equal(bits(ws), bits(np.zeros(2, np.float32)))
    # nothing at all
    s, ws, order, sid = weighted_sums(np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), 2)
    assert s.shape == (2, 3) and not s.any() and not ws.any() and order.size == 0
    assert imbalance_ref([2, 2], 2) == 1.0 and imbalance_ref([3, 1], 2) == 1.25


def test_vectorised_reference_is_the_literal_loop():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((700, 5)).astype(np.float32)
    w = full_mantissa_weights(700)
    ids = rng.integers(-1, 9, 700)                   # -1 and 8 are outside [0, 8)
    sums, wsum, order, sid = weighted_sums(x, w, ids, 8)
    ls, lw = weighted_sums_loop(x, w, ids, 8)
    assert np.array_equal(bits(sums), bits(ls)) and np.array_equal(bits(wsum), bits(lw))
    key = np.where((ids >= 0) & (ids < 8), ids, 8)
    assert np.array_equal(order, np.argsort(key, kind="stable")) and np.array_equal(sid, key[order])


def test_data_tells_the_contract_from_its_two_rounding_neighbour():
    """On the weights the GPU tests use the single-rounding sums differ from fl(x * w) + s: data on which they
    agreed could not tell which of the two a kernel computes."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((3000, 64)).astype(np.float32)
    w = full_mantissa_weights(3000)
    assert w.min() >= 0.25 and w.max() < 4 and (bits(w) & 0x7fffff).astype(bool).mean() > 0.99
    ids = rng.integers(0, 32, 3000)
    one, ws1, _, _ = weighted_sums(x, w, ids, 32)
    two, ws2, _, _ = weighted_sums_two_roundings(x, w, ids, 32)
    assert np.array_equal(bits(ws1), bits(ws2))
    differ = (bits(one) != bits(two)).mean()
    assert differ > 0.5, differ                      # in most sums, not in one lucky place


# ---- 2. host logic of ops.Kmeans.train(weights=) == the straight-line loop ------------------------------
def test_cold_and_warm_start_match_the_loop(wbe, golden, oracle):
    x, y = golden["a_x"], golden["b_x"]
    w = full_mantissa_weights(x.shape[0])
    km = _train(wbe, x, w, 64, 5)
    r1 = weighted_kmeans_ref(x, w, 64, 5)
    _same(km, r1)
    assert np.array_equal(km._last_assign.numpy(), r1.assign)
    # and the weights matter: the unweighted training ends elsewhere
    assert not np.array_equal(bits(km.centroids), bits(oracle.kmeans_train(x, 64, niter=5).centroids))
    w2 = full_mantissa_weights(y.shape[0], seed=21)
    km2 = _train(wbe, y, torch.from_numpy(w2).double(), 64, 5, init_centroids=km.centroids)   # any float dtype, a tensor
    _same(km2, weighted_kmeans_ref(y, w2, 64, 5, init=r1.centroids))


def test_subsampled_training_permutes_the_weights_with_the_rows(wbe, golden, oracle):
    x = golden["a_x"][:1200, :16].copy()
    w = full_mantissa_weights(1200)
    km = _train(wbe, x, w, 24, 3, max_points_per_centroid=2)          # 48 of 1200 rows
    r = weighted_kmeans_ref(x, w, 24, 3, max_points_per_centroid=2)
    _same(km, r)
    # weights left in their places (not permuted) give another result: the check above can tell
    perm = oracle.rand_perm(1200, 1234)[:48]
    wrong = w.copy()
    wrong[perm] = w[:48]
    assert not np.array_equal(bits(weighted_kmeans_ref(x, wrong, 24, 3, max_points_per_centroid=2).centroids), bits(r.centroids))


def test_cluster_whose_members_all_weigh_zero_is_reseeded(wbe, golden, oracle):
    x = golden["a_x"][:1500].copy()
    init = x[np.arange(48) * 31].copy()
    w = full_mantissa_weights(1500)
    ids0, _ = oracle.assign(x, init)
    planted = int(np.bincount(ids0, minlength=48).argmax())
    w[ids0 == planted] = 0.0                          # has members, weighs nothing
    km = _train(wbe, x, w, 48, 4, init_centroids=init)
    r = weighted_kmeans_ref(x, w, 48, 4, init=init)
    assert r.nsplit[0] >= 1
    _same(km, r)


def test_ns_equal_k_returns_the_rows(wbe):
    x = (np.random.default_rng(0).standard_normal((10, 4)) * 3).astype(np.float32)
    w = full_mantissa_weights(10)
    km = _train(wbe, x, w, 10, 3)
    assert np.array_equal(bits(km.centroids), bits(x)) and km.iteration_stats[0]["nsplit"] == 0
    _same(km, weighted_kmeans_ref(x, w, 10, 3))
    # ... also when the subsample is what makes ns == k
    x = (np.random.default_rng(1).standard_normal((40, 4)) * 3).astype(np.float32)
    km = _train(wbe, x, full_mantissa_weights(40), 10, 3, max_points_per_centroid=1)
    _same(km, weighted_kmeans_ref(x, full_mantissa_weights(40), 10, 3, max_points_per_centroid=1))


def test_spherical_weighted_matches_the_loop(golden, oracle):
    x = golden["a_x"][:900].copy()
    w = full_mantissa_weights(900)
    km = _train(SphericalWeightedOracleBackend(), x, w, 32, 4, spherical=True)
    _same(km, weighted_kmeans_ref(x, w, 32, 4, spherical=True))
    assert np.abs(np.linalg.norm(km.centroids.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_unit_weights_are_the_unweighted_training(wbe, golden):
    from audio_tokens_amd.ops import Kmeans
    x = golden["a_x"]
    init = x[np.arange(64) * 17].copy()
    init[40] = init[3]                                # an empty cluster in iteration 0: the repair is compared too
    for kw in (dict(), dict(init_centroids=init)):
        plain = Kmeans(64, 64, niter=4, backend=wbe)
        plain.train(x, **kw)
        ones = _train(wbe, x, np.ones(x.shape[0]), 64, 4, **kw)
        assert np.array_equal(bits(ones.centroids), bits(plain.centroids))
        assert np.array_equal(bits(ones.obj), bits(plain.obj))
        for a, b in zip(ones.iteration_stats, plain.iteration_stats):
            assert (a["obj"], a["nsplit"], a["imbalance_factor"]) == (b["obj"], b["nsplit"], b["imbalance_factor"])
    assert plain.iteration_stats[0]["nsplit"] >= 1


# ---- 3. the call surface ------------------------------------------------------------------------------------
def test_weights_are_keyword_only_and_checked(wbe, golden):
    from audio_tokens_amd.ops import Kmeans
    x = golden["a_x"][:400].copy()
    w = np.ones(400, np.float32)
    km = Kmeans(64, 8, niter=2, backend=wbe)
    with pytest.raises(ValueError, match="one per row"):
        km.train(x, weights=w[:399])
    with pytest.raises(ValueError, match="one per row"):
        km.train(x, weights=np.ones((400, 1), np.float32))
    for bad in (np.nan, np.inf, -1.0):
        wb = w.copy()
        wb[123] = bad
        with pytest.raises(ValueError, match="finite and not negative"):
            km.train(x, weights=wb)
    wz = w.copy()
    wz[5], wz[6] = 0.0, -0.0                          # both are "not negative"
    km.train(x, weights=wz)
    # check_finite=False reads nothing and follows the formula
    wn = w.copy()
    wn[0] = -0.5
    km.train(x, weights=wn, check_finite=False)
    # train(x, c) keeps its meaning: the second positional argument is init_centroids
    init = x[:8].copy()
    km.train(x, init)
    ref = Kmeans(64, 8, niter=2, backend=wbe)
    ref.train(x, init_centroids=init)
    assert np.array_equal(bits(km.centroids), bits(ref.centroids))
    with pytest.raises(TypeError):
        km.train(x, None, True, True, w)


def test_backend_without_the_method_raises_at_the_call(golden):
    from audio_tokens_amd.ops import Kmeans
    x = golden["a_x"][:400].copy()
    km = Kmeans(64, 8, niter=2, backend=OracleBackend())          # constructing is fine
    km.train(x)
    with pytest.raises(NotImplementedError, match="centroid_accum_weighted"):
        km.train(x, weights=np.ones(400, np.float32))


def test_weight_sum_of_at_most_k_with_an_empty_cluster_raises(wbe, golden):
    from audio_tokens_amd.ops import Kmeans
    x = golden["a_x"][:400].copy()
    init = x[:8].copy()
    init[5] = init[2]                                 # cluster 5 receives nobody
    km = Kmeans(64, 8, niter=1, backend=wbe)
    with pytest.raises(RuntimeError, match="weights"):
        km.train(x, init_centroids=init, weights=np.full(400, 1.0 / 400, np.float32))    # sum 1: no cluster outweighs one point


# ---- 4. world_size 2 under gloo -----------------------------------------------------------------------------
def _exact_data():
    """Rows that are multiples of 2^-8 below 4 in magnitude and integer weights 0 .. 3: every product and every sum
    of the training is exact in float32, so the order in which two shards' partials are added cannot show."""
    x = np.load(G / "kmeans.npz")["a_x"]
    x = (np.round(x * 8 * 256) / 256).astype(np.float32)
    w = np.random.default_rng(5).integers(0, 4, x.shape[0]).astype(np.float32)
    return x, w


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
        (x, w), cut = _exact_data(), 900
        sl = slice(0, cut) if rank == 0 else slice(cut, None)
        out = []
        for mppc in (256, 8):                         # whole set; subsampled (512 of the rows, spread over both ranks)
            km = Kmeans(64, 64, niter=4, distributed=True, backend=WeightedOracleBackend(), max_points_per_centroid=mppc)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                km.train(x[sl], weights=w[sl])
            out.append((km.centroids.copy(), [s["nsplit"] for s in km.iteration_stats], km.obj.copy()))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_sharded_weighted_kmeans_gloo_world2(wbe, oracle):
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
    x, w = _exact_data()
    assert x.shape[0] > 8 * 64
    for i, mppc in enumerate((256, 8)):
        km = _train(wbe, x, w, 64, 4, max_points_per_centroid=mppc)
        r = weighted_kmeans_ref(x, w, 64, 4, max_points_per_centroid=mppc)
        _same(km, r)
        for rank, out in res:
            cent, nsplit, obj = out[i]
            assert np.array_equal(bits(cent), bits(km.centroids)), f"rank {rank} differs from the single-process run"
            assert nsplit == r.nsplit
            assert np.array_equal(bits(obj), bits(km.obj))
