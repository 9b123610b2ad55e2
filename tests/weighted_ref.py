"""CPU reference of the weighted centroid sums and of weighted k-means (at_centroid_accum_weighted_f32,
ops.Kmeans.train(x, weights=w)), numpy only.  TEST ONLY.

The contract: for the members i0 < i1 < ... of a cluster, in ascending row,
    sums[c][f] = the chain s <- fmaf(x[i][f], w[i], s) from +0, one rounding per member (fma32 of spherical_ref.py),
    wsum[c]    = the chain s <- s + w[i] from +0, plain float32 adds.
Everything behind the sums is the unweighted recipe with wsum in the counts' place.  Its provenance is faiss'
Clustering::train_encoded as recalled, not verified faiss output."""
import numpy as np
import torch

import oracle
from centroid_sums_ref import finalize
from oracle_backend import OracleBackend
from spherical_ref import SphericalOracleBackend, fma32, renorm_ref, search_ip_ref


WEIGHT_SEED = 20          # chosen so that the data tells the contract from its neighbour (test_weighted_ref.py)


def full_mantissa_weights(n, seed=WEIGHT_SEED):
    """float32 weights in [0.25, 4) with random 23-bit mantissas."""
    rng = np.random.default_rng(seed)
    mant = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    expo = rng.integers(125, 129, n, dtype=np.uint32)           # 2^-2 .. 2^1
    return ((expo << np.uint32(23)) | mant).view(np.float32)


def _member_lists(ids, k):
    """-> (key, order, rank, length): the stable (cluster, row) order and every row's position in its own list."""
    ids = np.asarray(ids, dtype=np.int64)
    valid = (ids >= 0) & (ids < k)
    key = np.where(valid, ids, k)
    order = np.argsort(key, kind="stable")
    length = np.bincount(key, minlength=k + 1)
    start = np.cumsum(length) - length
    rank = np.empty(ids.size, np.int64)
    rank[order] = np.arange(ids.size) - start[key[order]]
    return key, order, rank, length


def _chains(x, w, ids, k, step):
    """The two chains with `step(x_rows, w_rows, s)` for the features; one numpy call per list position, all the
    clusters that have a member at that position side by side (a cluster's members still meet in ascending row)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    n, d = x.shape
    assert w.shape == (n,) and np.asarray(ids).shape == (n,)
    key, order, rank, length = _member_lists(ids, k)
    sums = np.zeros((k, d), np.float32)
    wsum = np.zeros(k, np.float32)
    by_rank = np.argsort(rank[order], kind="stable")          # positions of `order`, grouped by list position
    rows_by_rank = order[by_rank]
    rows_by_rank = rows_by_rank[key[rows_by_rank] < k]
    cuts = np.cumsum(np.bincount(rank[rows_by_rank], minlength=1))
    lo = 0
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for hi in cuts:
            rows = rows_by_rank[lo:hi]
            lo = hi
            c = key[rows]                                      # distinct clusters: one member each at this position
            sums[c] = step(x[rows], w[rows, None], sums[c])
            wsum[c] = wsum[c] + w[rows]
    return sums, wsum, order.astype(np.uint32), key[order].astype(np.uint32)


def weighted_sums(x, w, ids, k):
    """-> (sums [k, d] float32, wsum [k] float32, order uint32 [n], sorted_ids uint32 [n]); ids outside [0, k) are
    parked in a trailing bucket k, order / sorted_ids as centroid_sums_ref.sequential_sums returns them."""
    return _chains(x, w, ids, k, fma32)


def weighted_sums_two_roundings(x, w, ids, k):
    """The neighbour the contract is NOT: fl(x * w), then a float32 add (what c[j] += xi[j] * w compiles to without
    contraction)."""
    return _chains(x, w, ids, k, lambda xr, wr, s: s + xr * wr)


def weighted_sums_loop(x, w, ids, k):
    """weighted_sums as the literal loop over the rows (slow; holds the vectorised form in test_weighted_ref.py)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    sums = np.zeros((k, x.shape[1]), np.float32)
    wsum = np.zeros(k, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i, c in enumerate(np.asarray(ids)):
            if 0 <= c < k:
                sums[c] = fma32(x[i], w[i], sums[c])
                wsum[c] = wsum[c] + w[i]
    return sums, wsum


def imbalance_ref(hassign, k):
    h = np.asarray(hassign, dtype=np.float64)
    return float((h * h).sum() * k / (h.sum() ** 2))


class WeightedResult:
    __slots__ = ("centroids", "obj", "nsplit", "imbalance", "assign")


def weighted_kmeans_ref(x, w, k, niter, init=None, seed=1234, spherical=False, max_points_per_centroid=256):
    """Kmeans(d, k, niter=niter, spherical=spherical).train(x, init_centroids=init, weights=w), one straight-line loop."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    n, d = x.shape
    assert n >= k and w.shape == (n,)
    r = WeightedResult()
    r.obj, r.nsplit, r.imbalance, r.assign = [], [], [], None
    if n > max_points_per_centroid * k:
        perm = oracle.rand_perm(n, seed)[:max_points_per_centroid * k]
        xs, ws = x[perm], w[perm]                               # the weights follow the rows
    else:
        xs, ws = x, w
    ns = xs.shape[0]
    if ns == k:
        r.centroids, r.obj, r.nsplit, r.imbalance = xs.copy(), [0.0], [0], [1.0]
        return r
    cent = np.array(init, dtype=np.float32) if init is not None else xs[oracle.rand_perm(ns, seed + 1)[:k]]
    assert cent.shape == (k, d)
    if spherical:
        cent = renorm_ref(cent)
    for _ in range(niter):
        ids, dis = search_ip_ref(xs, cent) if spherical else oracle.assign(xs, cent)
        r.obj.append(float(np.float32(dis.astype(np.float64).sum())))      # unweighted
        sums, wsum, _, _ = weighted_sums(xs, ws, ids, k)
        cent, hassign = finalize(sums[None], wsum[None])
        r.imbalance.append(imbalance_ref(hassign, k))
        nsplit = 0
        if (hassign == 0).any():
            assert (hassign > 1).any(), "no donor: oracle.split_clusters would not return"
            nsplit, hassign, cent = oracle.split_clusters(hassign, cent, ns)
        r.nsplit.append(int(nsplit))
        if spherical:
            cent = renorm_ref(cent)
        r.assign = ids
    r.centroids = cent
    return r


class WeightedOracleBackend(OracleBackend):
    """OracleBackend with centroid_accum_weighted from the reference above."""

    def centroid_accum_weighted(self, x, w, ids, k, out=None, want_order=False):
        x = self._f32(x).numpy()
        d = x.shape[1]
        sums, wsum, _, _ = weighted_sums(x, self._f32(w).numpy(), ids.numpy(), k)
        part = torch.from_numpy(np.concatenate([sums.ravel(), wsum]))
        if out is not None:
            out[: k * d + k] = part
            part = out
        return (part, None) if want_order else part

    def split_clusters_device(self, hassign, cent, n, nsplit_out):
        # the device kernel's exit: no cluster with a positive acceptance probability, nobody to split -> -1
        # (the host loop it stands in for would draw for ever)
        h = hassign.numpy()
        if (h == 0).any() and not (h > 1).any():
            nsplit_out[0] = -1
            return
        super().split_clusters_device(hassign, cent, n, nsplit_out)


class SphericalWeightedOracleBackend(WeightedOracleBackend):
    assign_ip = SphericalOracleBackend.assign_ip
    renorm_rows = SphericalOracleBackend.renorm_rows
