"""at_centroid_accum_weighted_f32 and Kmeans.train(x, weights=w) on the MI355X against tests/weighted_ref.py, bit for bit:
every member-list length at which a loop of csrc/waccum.hip changes course, at every lane width and alignment of its
plan; weights that must not be mistaken (0, -0, a denormal, an overflow); the forms of a call; and whole trainings.

Every comparison is on bit patterns (where an infinity is planted the NaN masks are compared too), the objective
included: the device sums the n float32 distances in float64 in a fixed tree, the reference in numpy's order, and both
narrow to float32 -- the float64 sums agree to n * 2^-53 relative, so the narrowed values differ only if a sum lies
that close to a float32 rounding boundary, which on this fixed data it does not.  One figure is not: the imbalance
factor, k doubles summed in a fixed but unspecified tree (relative k * 2^-52).  Every call writes into a buffer filled
with NaN."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from centroid_sums_ref import finalize, ids_with_lengths
from device_rows import rows_one_float_off
from weighted_ref import full_mantissa_weights, weighted_kmeans_ref, weighted_sums

pytestmark = pytest.mark.gpu

K_LADDER = 40
FLT_MAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, ref, what, nan_ok=False):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    differ = bits(got) != bits(ref)
    if nan_ok:
        gn, rn = np.isnan(got), np.isnan(ref)
        assert np.array_equal(gn, rn), f"{what}: NaN masks differ, first at {np.argwhere(gn != rn)[0]}"
        differ &= ~rn
    bad = np.argwhere(differ)
    assert bad.size == 0, (f"{what}: {len(bad)} of {got.size} values differ, first at {bad[0]}: "
                           f"got {got[tuple(bad[0])]!r} want {ref[tuple(bad[0])]!r}")


def _dev(be, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(be.device)


def _out(be, k, d):
    return torch.full((k * d + k,), float("nan"), dtype=torch.float32, device=be.device)


def _verify(got, ref, k, d, want_order, label, nan_ok=False):
    sums, wsum, r_order, r_sorted = ref
    part, pair = got if want_order else (got, None)
    p = part.cpu().numpy()
    _same(p[: k * d].reshape(k, d), sums, f"{label}: sums", nan_ok)
    _same(p[k * d: k * d + k], wsum, f"{label}: weight sums", nan_ok)
    if want_order:
        nv = int((r_sorted < k).sum())
        order = pair[0].cpu().numpy().view(np.uint32)
        assert np.array_equal(order[:nv], r_order[:nv]), f"{label}: member order"
        assert np.array_equal(np.sort(order[nv:]), np.sort(r_order[nv:])), f"{label}: trailing bucket"
        assert np.array_equal(pair[1].cpu().numpy().view(np.uint32), r_sorted), f"{label}: sorted ids"


# ---- the ladder ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _limits():
    from audio_tokens_amd.backend import HipBackend
    lim = HipBackend.waccum_limits()
    assert lim["short_batch_wide"] < lim["short_batch"] < 63 and 129 < lim["long_list"] <= lim["ring_chunk"]
    return lim


@functools.lru_cache(maxsize=None)
def _ladder_ids():
    """-> (ids, lengths, special): K_LADDER clusters whose member lists have every length at which a loop changes
    course, scattered over the rows; two ids outside [0, k) among them; the clusters with planted weights."""
    lim = _limits()
    rb, rbw, L, C = lim["short_batch"], lim["short_batch_wide"], lim["long_list"], lim["ring_chunk"]
    lengths = [0, 1, 2, 63, 64, 65, 127, 128, 129, rbw - 1, rbw, rbw + 1, rb - 1, rb, rb + 1, 2 * rb, 2 * rb + 1,
               L, L + 1, C + 1, 2 * C + 1, C + 64, C + 16 + 3]
    rng = np.random.default_rng(41)
    lengths += list(rng.integers(150, 400, K_LADDER - len(lengths)))
    assert len(lengths) == K_LADDER
    ids, n = ids_with_lengths(lengths, rng, scatter=True)
    parked = rng.choice(np.flatnonzero(ids == K_LADDER - 1), 2, replace=False)    # (one of the 150 .. 400 lists)
    ids[parked[0]], ids[parked[1]] = -1, K_LADDER + 5
    lengths[K_LADDER - 1] -= 2
    special = dict(zero=K_LADDER - 2, overflow_short=K_LADDER - 3, overflow_long=lengths.index(C + 1))
    return ids, lengths, special


@functools.lru_cache(maxsize=None)
def _ladder_case(d):
    """-> (x, w, ids, reference) at width d: full-mantissa weights, and planted: 0, -0 and a denormal in the long and
    in short lists, one cluster whose members all weigh 0, FLT_MAX / 2 on rows of 8.0 in a short and in a long list
    (the sums, and three of them the weight sum, overflow to +inf by the formula)."""
    ids, lengths, special = _ladder_ids()
    n = ids.size
    rng = np.random.default_rng(1000 + d)
    x = rng.standard_normal((n, d)).astype(np.float32)
    w = full_mantissa_weights(n)
    for c, vals in ((lengths.index(2 * _limits()["ring_chunk"] + 1), (0.0, -0.0, 1e-41)), (5, (1e-41, -0.0)),
                    (K_LADDER - 4, (0.0, 1e-45))):
        rows = np.flatnonzero(ids == c)
        w[rows[np.arange(len(vals)) * 7 % rows.size]] = np.array(vals, np.float32)
    w[ids == special["zero"]] = 0.0
    for c in (special["overflow_short"], special["overflow_long"]):
        rows = np.flatnonzero(ids == c)[[3, 40, 41]]
        w[rows] = FLT_MAX / 2
        x[rows] = 8.0
    ref = weighted_sums(x, w, ids, K_LADDER)
    assert np.isinf(ref[0][special["overflow_long"]]).all() and np.isinf(ref[1][special["overflow_short"]])
    assert not np.isnan(ref[0]).any() and ref[1][special["zero"]] == 0 and lengths[special["zero"]] > 0
    return x, w, ids, ref


@pytest.fixture(scope="module", autouse=True)
def _release_cached_cases():
    yield
    _ladder_case.cache_clear()


@pytest.mark.parametrize("d", [64, 128, 8, 50, 6, 640])
def test_length_ladder(be, d):
    """d = 64, 8: one feature per lane; 128: two; 640: four (the narrower row batch); 50, 6: the scalar-lane form that
    walks the long lists too (d % 4 != 0)."""
    x, w, ids, ref = _ladder_case(d)
    got = be.centroid_accum_weighted(_dev(be, x), _dev(be, w), _dev(be, ids), K_LADDER, out=_out(be, K_LADDER, d), want_order=True)
    _verify(got, ref, K_LADDER, d, True, f"ladder d={d}", nan_ok=True)
    # behind the sums: the existing finalize with the weight sums in the counts' place; the all-zero cluster comes out
    # as a zero row with hassign 0 (what split_clusters re-seeds)
    part = got[0]
    nonfinite = ~np.isfinite(ref[1]) | ~np.isfinite(ref[0]).all(axis=1)
    cent, h = be.centroid_finalize(part, K_LADDER, d)
    r_cent, r_h = finalize(ref[0][None], ref[1][None])
    _same(h.cpu().numpy(), r_h, "hassign", nan_ok=True)
    _same(cent.cpu().numpy()[~nonfinite], r_cent[~nonfinite], "finalize")
    zero = _ladder_ids()[2]["zero"]
    assert r_h[zero] == 0 and not r_cent[zero].any()


@pytest.mark.parametrize("d", [64, 128, 640])
def test_unaligned_rows_give_the_same_bits(be, d):
    x, w, ids, ref = _ladder_case(d)
    xt = rows_one_float_off(x, be.device)
    got = be.centroid_accum_weighted(xt, _dev(be, w), _dev(be, ids), K_LADDER, out=_out(be, K_LADDER, d), want_order=True)
    _verify(got, ref, K_LADDER, d, True, f"unaligned d={d}", nan_ok=True)


@pytest.mark.parametrize("d", [4, 8])
def test_more_long_lists_than_workgroups(be, d):
    """66 lists of long_list + 1 members on the long-list kernel's grid of 64 workgroups per 4-feature slice (d = 4: one
    slice, 8: two): two workgroups of a slice sum a second list each, from a ring the first one has been through."""
    L, k = _limits()["long_list"], 70
    lengths = [L + 1] * 66 + [3, 0, 3, 0]
    rng = np.random.default_rng(70 + d)
    ids, n = ids_with_lengths(lengths, rng, scatter=True)
    assert n // (L + 1) > 64 and sum(m > L for m in lengths) > 64      # (the grid is min(n // (L + 1), 64))
    x = rng.standard_normal((n, d)).astype(np.float32)
    w = full_mantissa_weights(n)
    got = be.centroid_accum_weighted(_dev(be, x), _dev(be, w), _dev(be, ids), k, out=_out(be, k, d), want_order=True)
    _verify(got, weighted_sums(x, w, ids, k), k, d, True, f"66 long lists, d={d}")


def test_call_forms(be):
    d = 64
    x, w, ids, ref = _ladder_case(d)
    xt, wt, it = _dev(be, x), _dev(be, w), _dev(be, ids)
    # without the order; without out=
    got = be.centroid_accum_weighted(xt, wt, it, K_LADDER)
    assert got.shape == (K_LADDER * d + K_LADDER,)
    _verify(got, ref, K_LADDER, d, False, "no order, no out", nan_ok=True)
    # two calls back to back, read afterwards: the second one's lists are in the same workspace as the first one's
    rng = np.random.default_rng(9)
    ids2 = rng.permutation(ids)
    w2 = full_mantissa_weights(ids.size, seed=23)
    ref2 = weighted_sums(x, w2, ids2, K_LADDER)
    o1, o2 = _out(be, K_LADDER, d), _out(be, K_LADDER, d)
    g1 = be.centroid_accum_weighted(xt, wt, it, K_LADDER, out=o1, want_order=True)
    g2 = be.centroid_accum_weighted(xt, _dev(be, w2), _dev(be, ids2), K_LADDER, out=o2, want_order=True)
    assert g1[0] is o1 and g2[0] is o2
    _verify(g1, ref, K_LADDER, d, True, "first of two", nan_ok=True)
    _verify(g2, ref2, K_LADDER, d, True, "second of two")
    # a call on a second stream behind one on the first: it waits for the workspace, not for the caller
    side = torch.cuda.Stream(device=be.device)
    w2t, ids2t = _dev(be, w2), _dev(be, ids2)
    o3, o4 = _out(be, K_LADDER, d), _out(be, K_LADDER, d)
    torch.cuda.synchronize(be.device)
    g3 = be.centroid_accum_weighted(xt, wt, it, K_LADDER, out=o3, want_order=True)
    with torch.cuda.stream(side):
        g4 = be.centroid_accum_weighted(xt, w2t, ids2t, K_LADDER, out=o4, want_order=True)
    torch.cuda.synchronize(be.device)
    _verify(g3, ref, K_LADDER, d, True, "first stream", nan_ok=True)
    _verify(g4, ref2, K_LADDER, d, True, "second stream")


def test_one_cluster_and_no_rows(be):
    rng = np.random.default_rng(2)
    lim = _limits()
    n, d = lim["ring_chunk"] + 70, 12
    x = rng.standard_normal((n, d)).astype(np.float32)
    w = full_mantissa_weights(n)
    ids = np.zeros(n, np.int64)
    got = be.centroid_accum_weighted(_dev(be, x), _dev(be, w), _dev(be, ids), 1, out=_out(be, 1, d), want_order=True)
    _verify(got, weighted_sums(x, w, ids, 1), 1, d, True, "k = 1")
    # n = 0: every sum is +0, nothing is read
    empty = torch.empty((0, d), dtype=torch.float32, device=be.device)
    got = be.centroid_accum_weighted(empty, empty[:, 0].contiguous(), torch.empty(0, dtype=torch.int64, device=be.device), 3,
                                     out=_out(be, 3, d), want_order=True)
    _same(got[0].cpu().numpy(), np.zeros(3 * d + 3, np.float32), "n = 0")
    assert got[1][0].numel() == 0 and got[1][1].numel() == 0


def test_abi_argument_errors(be):
    from audio_tokens_amd import _lib
    lib, h = be.lib, be.ctx.handle
    x = torch.zeros((4, 8), dtype=torch.float32, device=be.device)
    w = torch.ones(4, dtype=torch.float32, device=be.device)
    ids = torch.zeros(4, dtype=torch.int64, device=be.device)
    out = torch.zeros(2 * 8 + 2, dtype=torch.float32, device=be.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    sums, wsums = p(out), ctypes.c_void_p(out.data_ptr() + 4 * 16)
    good = [h, p(x), p(w), 4, 8, p(ids), 2, sums, wsums, None, None, None]

    def call(**kw):
        names = ["ctx", "x", "w", "n", "d", "ids", "k", "sums", "wsums", "order", "sorted", "stream"]
        a = list(good)
        for name, v in kw.items():
            a[names.index(name)] = v
        return lib.at_centroid_accum_weighted_f32(*a)
    assert call() == 0
    for kw, msg in ((dict(ctx=None), "ctx is null"), (dict(n=-1), "bad sizes"), (dict(n=2 ** 32), "bad sizes"),
                    (dict(d=0), "bad sizes"), (dict(k=0), "bad sizes"), (dict(k=1 << 30), "bad sizes"),
                    (dict(sums=None), "null pointer"), (dict(wsums=None), "null pointer"), (dict(x=None), "null pointer"),
                    (dict(w=None), "null pointer"), (dict(ids=None), "null pointer")):
        assert call(**kw) == -1, kw
        assert "at_centroid_accum_weighted_f32" in _lib.last_error() and msg in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize(be.device)


# ---- trainings on the device ---------------------------------------------------------------------------------
def _rows(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((max(8, n // 60), d)).astype(np.float32)
    x = centres[rng.integers(0, centres.shape[0], n)] + np.float32(0.3) * rng.standard_normal((n, d)).astype(np.float32)
    return x.astype(np.float32)


def _train(be, x, w, k, niter, prune=True, **kw):
    from audio_tokens_amd.ops import Kmeans
    ctor = {n: kw.pop(n) for n in ("spherical", "max_points_per_centroid") if n in kw}
    km = Kmeans(x.shape[1], k, niter=niter, backend=be, **ctor)
    km.prune = prune
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km.train(x, weights=w, **kw)
    return km


def _same_training(km, r, k, label):
    _same(km.centroids, r.centroids, f"{label}: centroids")
    st = km.iteration_stats
    assert [s["nsplit"] for s in st] == r.nsplit, label
    obj, want = km.obj, np.array(r.obj, np.float32)
    print(f"{label}: obj {obj.tolist()} want {want.tolist()}")
    _same(obj, want, f"{label}: objective")
    imb, want = np.array([s["imbalance_factor"] for s in st]), np.array(r.imbalance)
    print(f"{label}: imbalance rel. diff {(np.abs(imb - want) / want).max():.3g}, bound {k * 2.0 ** -52:.3g}")
    assert (np.abs(imb - want) <= k * 2.0 ** -52 * want).all(), label


@pytest.mark.parametrize("n,d,k,niter", [(3000, 64, 32, 4), (2500, 50, 17, 3)])
def test_training_cold_and_warm(be, oracle, n, d, k, niter):
    x, y = _rows(n, d, 1), _rows(n, d, 2)
    w, w2 = full_mantissa_weights(n), full_mantissa_weights(n, seed=21)
    km = _train(be, x, w, k, niter)
    r1 = weighted_kmeans_ref(x, w, k, niter)
    _same_training(km, r1, k, "cold")
    assert np.array_equal(km._last_assign.cpu().numpy(), r1.assign)
    km2 = _train(be, y, _dev(be, w2, np.float64), k, niter, init_centroids=km.centroids)     # device, float64
    _same_training(km2, weighted_kmeans_ref(y, w2, k, niter, init=r1.centroids), k, "warm")


def test_training_subsampled(be, oracle):
    x, w = _rows(3000, 64, 3), full_mantissa_weights(3000)
    km = _train(be, x, w, 32, 3, max_points_per_centroid=40)              # 1280 of 3000 rows
    _same_training(km, weighted_kmeans_ref(x, w, 32, 3, max_points_per_centroid=40), 32, "subsampled")


def test_training_spherical(be, oracle):
    x, w = _rows(1500, 64, 4), full_mantissa_weights(1500)
    km = _train(be, x, w, 24, 3, spherical=True)
    _same_training(km, weighted_kmeans_ref(x, w, 24, 3, spherical=True), 24, "spherical")


def test_training_zero_weight_cluster_is_reseeded_on_the_device(be, oracle):
    x, w = _rows(3000, 64, 5), full_mantissa_weights(3000)
    init = x[np.arange(32) * 90].copy()
    ids0, _ = oracle.assign(x, init)
    w[ids0 == int(np.bincount(ids0, minlength=32).argmax())] = 0.0
    r = weighted_kmeans_ref(x, w, 32, 3, init=init)
    assert r.nsplit[0] >= 1
    _same_training(_train(be, x, w, 32, 3, init_centroids=init), r, 32, "zero-weight cluster")


@functools.lru_cache(maxsize=None)
def _pruned_case():
    """The smallest shape _PrunedSweep.applies admits: d = 64, k = 1024 (the next condition, at most 512 groups of 32
    centroids, is far off), 4096 rows."""
    n, d, k = 4096, 64, 1024
    x = _rows(n, d, 6)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    w = full_mantissa_weights(n)
    return x, w, k, weighted_kmeans_ref(x, w, k, 4)


@pytest.mark.parametrize("prune", [True, False])
def test_training_at_the_smallest_pruned_shape(be, oracle, prune):
    from audio_tokens_amd.ops import _PrunedSweep
    x, w, k, r = _pruned_case()
    assert _PrunedSweep.applies(be, x.shape[1], k, x.shape[0])
    assert not _PrunedSweep.applies(be, x.shape[1], k, x.shape[0] - 1) and not _PrunedSweep.applies(be, x.shape[1], k - 1, x.shape[0])
    _same_training(_train(be, x, w, k, 4, prune=prune), r, k, f"prune={prune}")


def test_unit_weights_equal_no_weights_on_the_device(be):
    from audio_tokens_amd.ops import Kmeans
    x, _, k, _ = _pruned_case()
    plain = Kmeans(x.shape[1], k, niter=4, backend=be)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain.train(x)
    ones = _train(be, x, np.ones(x.shape[0]), k, 4)
    _same(ones.centroids, plain.centroids, "centroids")
    _same(ones.obj, plain.obj, "obj")
    for a, b in zip(ones.iteration_stats, plain.iteration_stats):
        assert (a["obj"], a["nsplit"], a["imbalance_factor"]) == (b["obj"], b["nsplit"], b["imbalance_factor"])
    assert np.array_equal(ones.index.search(x[:100], 1)[1], plain.index.search(x[:100], 1)[1])


def test_weights_checked_on_the_device(be):
    from audio_tokens_amd.ops import Kmeans
    x = _rows(400, 64, 7)
    km = Kmeans(64, 8, niter=1, backend=be)
    for bad in (np.nan, np.inf, -1.0):
        w = np.ones(400, np.float32)
        w[17] = bad
        with pytest.raises(ValueError, match="finite and not negative"):
            km.train(x, weights=w)
    with pytest.raises(ValueError, match="one per row"):
        km.train(x, weights=np.ones(399, np.float32))
    init = x[:8].copy()
    init[5] = init[2]
    km.train(x, init_centroids=init, weights=np.full(400, 1.0 / 400, np.float32), sync=False)
    with pytest.raises(RuntimeError, match="weights"):
        km.iteration_stats
