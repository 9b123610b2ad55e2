"""Bit-exact reference of ops.IndexIVFFlat / at_ivf_search_f32, composed from knn_ref and the CPU oracle.

    lists   of the stored rows: column 0 of knn_ref(oracle, stored, centroids, 1)          (quantizer.assign)
    probes  of the queries:     the ids of knn_ref(oracle, x, centroids, min(nprobe, nlist)) (backend.knn; -1: no list)
    dis(i, r): knn_ref.distance_matrix with the query block padded to at least 20 rows (row 0 repeated), so that the
               oracle takes the expansion form whatever n is
    row i:  the k smallest (dis, id) over the stored rows whose list is >= 0 and among the probes of i.
No float64 anywhere."""
import numpy as np

from knn_ref import distance_matrix, knn_ref, select

EXPANSION_ROWS = 20   # the oracle's (faiss's) threshold between the direct and the expansion form


def ivf_lists(oracle, stored, centroids):
    """int64 [ntotal]: the list of every stored row, -1 for a row no centroid is listable for."""
    stored = np.ascontiguousarray(stored, dtype=np.float32)
    if stored.shape[0] == 0:
        return np.zeros(0, np.int64)
    return knn_ref(oracle, stored, centroids, 1)[1][:, 0].copy()


def ivf_probes(oracle, x, centroids, nprobe):
    """int64 [n, min(nprobe, nlist)]: the probed lists of every query, -1 in the slots with nothing to list."""
    centroids = np.ascontiguousarray(centroids, dtype=np.float32)
    return knn_ref(oracle, x, centroids, min(int(nprobe), centroids.shape[0]))[1]


def ivf_distances(oracle, x, stored):
    """(dis [n, ntotal] float32, listable [n, ntotal] bool) in the expansion form whatever n is."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    xp = x if n >= EXPANSION_ROWS else np.concatenate([x, np.repeat(x[:1], EXPANSION_ROWS - n, 0)], 0)
    dis, ok = distance_matrix(oracle, xp, stored)
    return dis[:n], ok[:n]


def ivf_select(dis, ok, lists, probes, k):
    """(D [n, k] float32, I [n, k] int64) from the distances, the stored rows' lists and the queries' probes."""
    lists = np.asarray(lists, np.int64)
    probes = np.asarray(probes, np.int64)
    mask = np.zeros(dis.shape, bool)
    for i in range(dis.shape[0]):
        mine = probes[i][probes[i] >= 0]
        mask[i] = (lists >= 0) & np.isin(lists, mine)
    return select(dis, ok & mask, int(k))


def ivf_search_ref(oracle, x, stored, lists, centroids, nprobe, k, distances=None):
    """IndexIVFFlat.search(x, k) on the CPU, bit for bit.  distances: ivf_distances(oracle, x, stored), if at hand."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    stored = np.ascontiguousarray(stored, dtype=np.float32)
    if x.shape[0] == 0 or stored.shape[0] == 0:
        return np.full((x.shape[0], k), np.inf, np.float32), np.full((x.shape[0], k), -1, np.int64)
    dis, ok = distances if distances is not None else ivf_distances(oracle, x, stored)
    return ivf_select(dis, ok, lists, ivf_probes(oracle, x, centroids, nprobe), k)


# ---- the tie constructions that test_ivf_ref.py and test_gpu_ivf.py share ------------------------------------------

def tie_case():
    """Seven distinct rows, each stored 40 times (row r carries value r % 7), spread over two lists in two ways: every
    copy of a value in ONE list (list = value % 2), and the copies of a value alternating between BOTH lists."""
    rng = np.random.default_rng(5)
    seven = (rng.integers(-8, 9, (7, 8)) / 8.0).astype(np.float32)
    assert len({tuple(r) for r in seven}) == 7
    stored = np.tile(seven, (40, 1))
    x = (rng.integers(-8, 9, (25, 8)) / 8.0).astype(np.float32)
    r = np.arange(stored.shape[0])
    inside = ((r % 7) % 2).astype(np.int64)
    across = ((r // 7) % 2).astype(np.int64)
    return x, stored, inside, across


def check_ties(D, I, full, allowed, k):
    """Every tie group is listed from its lowest allowed id on; only the group the cut falls in may be incomplete.
    Returns whether the cut fell inside a tie group for some row."""
    cut = False
    for i in range(D.shape[0]):
        assert np.all(np.diff(D[i]) >= 0)
        for v in np.unique(D[i]):
            listed = I[i][D[i] == v]
            group = np.flatnonzero((full[i] == v) & allowed[i])
            assert group.size >= 20 and np.array_equal(listed, group[:listed.size]), (k, i, v)
            if v != D[i, -1]:
                assert listed.size == group.size
            else:
                cut |= listed.size < group.size
    return cut
