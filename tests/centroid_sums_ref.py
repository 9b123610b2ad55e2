"""Plain reference of the centroid sums (at_centroid_accum_f32 / at_centroid_finalize_f32), numpy only.

The contract: for every cluster the fp32 sum of its member rows in ASCENDING row index, one add per member, starting
from +0.  np.add.at is unbuffered and walks the rows in order, so it is that sum (tests/test_centroid_sums_ref.py holds
it to the literal Python loop).  No float64 anywhere."""
import numpy as np


def sequential_sums(x, ids, k):
    """-> (sums [k, d] float32, counts [k] float32, order uint32 [n], sorted_ids uint32 [n]).

    ids outside [0, k) go to a trailing bucket k that no sum reads; order is the stable argsort of that key (rows by
    (cluster, row)), sorted_ids the key in that order."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    n, d = x.shape
    assert ids.shape == (n,)
    valid = (ids >= 0) & (ids < k)
    key = np.where(valid, ids, k)
    order = np.argsort(key, kind="stable")
    sums = np.zeros((k, d), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):          # (+inf + -inf, on purpose, in some cases)
        np.add.at(sums, ids[valid], x[valid])                   # unbuffered, ascending row: the sequential fp32 sum
    counts = np.bincount(key, minlength=k + 1)[:k].astype(np.float32)
    return sums, counts, order.astype(np.uint32), key[order].astype(np.uint32)


def ids_with_lengths(lengths, rng, scatter=True):
    """-> (ids int64 [n], n): cluster c has exactly lengths[c] members; with scatter they sit at random rows, so no
    member list is a contiguous range of rows."""
    lengths = np.asarray(lengths, dtype=np.int64)
    assert (lengths >= 0).all()
    ids = np.repeat(np.arange(lengths.size, dtype=np.int64), lengths)
    if scatter:
        ids = ids[rng.permutation(ids.size)]
    return ids, int(ids.size)


def finalize(parts_sums, parts_counts):
    """parts_sums [P, k, d], parts_counts [P, k] (part order) -> (centroids [k, d], counts [k]): counts and sums added
    in part order in fp32 starting from +0, then sum * (float32(1) / count), 0 where the count is 0."""
    parts_sums = np.asarray(parts_sums, dtype=np.float32)
    parts_counts = np.asarray(parts_counts, dtype=np.float32)
    tot = np.zeros(parts_sums.shape[1:], np.float32)
    cnt = np.zeros(parts_counts.shape[1:], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, c in zip(parts_sums, parts_counts):
            tot = tot + s
            cnt = cnt + c
        cent = np.zeros_like(tot)
        nz = cnt != 0
        cent[nz] = tot[nz] * (np.float32(1.0) / cnt[nz])[:, None]
    return cent, cnt


def sum_parts(parts):
    """parts [P, m] -> [m]: ((0 + parts[0]) + parts[1]) + ... in fp32."""
    tot = np.zeros(parts.shape[1], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in np.asarray(parts, dtype=np.float32):
            tot = tot + p
    return tot
