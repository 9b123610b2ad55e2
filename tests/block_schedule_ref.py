"""Numpy model of the block schedules of the exact filter sweep (csrc/exact_plan.h, the kernels in csrc/prune.hip):
sorted visiting-order keys -> a weight per 32-row tile -> a class per block of 1, 2 or 4 tiles -> the blocks in
descending class, ascending index within a class.  TEST ONLY.

    key      guess (k without one) << dbits | quantised distance  (guess_ref.visit_order_model's key, sorted, stable)
    weight   the largest distance field among the tile's rows, scaled to 8 bits (>> (dbits - 8) or << (8 - dbits));
             255 if a row of the tile has no guess, or if its first and last row belong to different clusters
    class    (largest weight among the block's tiles) >> 4
"""
import numpy as np

WEIGHT_MAX = 255
CLASS_BITS = 4


def make_keys(ids, dis, k, dbits=8):
    """keys int64 [n] as at_visit_order_f32 makes them, before the sort (float32 arithmetic)."""
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < k)
    top = np.float32((1 << dbits) - 1)
    if dis is None:
        r = np.zeros(ids.size, np.float32)
    else:
        r = np.sqrt(np.maximum(np.asarray(dis, np.float32), np.float32(0))) * (np.float32(0.5) * top)
    r = np.minimum(r, top).astype(np.uint32).astype(np.int64)
    return (np.where(ok, ids, k) << dbits) | r


def sorted_keys(ids, dis, k, dbits=8):
    """(keys int64 [n] sorted, order int64 [n]): the stable sort of at_visit_order_f32."""
    key = make_keys(ids, dis, k, dbits)
    order = np.argsort(key, kind="stable")
    return key[order], order


def tile_weights(keys, k, dbits=8):
    """int64 [ceil(n / 32)] from the sorted keys."""
    keys = np.asarray(keys, np.int64)
    # (the last tile filled up with its last row: neither its largest field nor its last cluster changes)
    kp = np.concatenate([keys, np.repeat(keys[-1:], -keys.size % 32)]).reshape(-1, 32)
    cluster, field = kp >> dbits, kp & ((1 << dbits) - 1)
    w = (field >> (dbits - 8) if dbits >= 8 else field << (8 - dbits)).max(axis=1)
    w[(cluster >= k).any(axis=1) | (cluster[:, 0] != cluster[:, -1])] = WEIGHT_MAX
    return w


def block_classes(weights, tiles):
    """int64 [ceil(len(weights) / tiles)]: the class of every block of `tiles` consecutive tiles."""
    w = np.asarray(weights, np.int64)
    return np.maximum.reduceat(w, np.arange(0, w.size, tiles)) >> (8 - CLASS_BITS)


def schedule(weights, tiles):
    """int64 [blocks]: the blocks in descending class, ascending index within a class."""
    return np.argsort(-block_classes(weights, tiles), kind="stable")


def is_schedule_of(table, classes):
    """table is a permutation of range(len(classes)) in which classes descend and indices ascend within a class."""
    table = np.asarray(table, np.int64)
    if not np.array_equal(np.sort(table), np.arange(len(classes))):
        return False
    cl = np.asarray(classes)[table]
    same = cl[1:] == cl[:-1]
    return bool((cl[1:] <= cl[:-1]).all() and (table[1:][same] > table[:-1][same]).all())
