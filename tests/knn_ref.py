"""Bit-exact reference of IndexFlatL2.search(x, k) / at_knn_f32, built from the CPU oracle.

oracle.assign(x, c[j:j+1]) is dis(i, j) exactly as at_assign_f32 computes it (the ascending fmaf chains, the direct form
for n < 20); it answers id -1 where the distance is not below +inf (NaN, overflow), and such a centroid is never listed.
Each row then lists the k smallest (dis, j) in lexicographic order, padded with (-1, +inf).  No float64 anywhere."""
import numpy as np


def distance_matrix(oracle, x, c):
    """(dis [n, k_c] float32, listable [n, k_c] bool): one oracle call per centroid column."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    c = np.ascontiguousarray(c, dtype=np.float32)
    n, kc = x.shape[0], c.shape[0]
    dis = np.empty((n, kc), np.float32)
    ok = np.empty((n, kc), bool)
    for j in range(kc):
        ids, dj = oracle.assign(x, c[j:j + 1])
        ok[:, j] = ids == 0
        dis[:, j] = dj
    return dis, ok


def select(dis, ok, k):
    """(D [n, k] float32, I [n, k] int64) from a distance matrix: the k smallest listable (dis, j) per row."""
    n, kc = dis.shape
    D = np.full((n, k), np.inf, np.float32)
    I = np.full((n, k), -1, np.int64)
    cols = np.arange(kc, dtype=np.int64)
    for i in range(n):
        keep = ok[i] & (dis[i] < np.float32(np.inf))
        di, ji = dis[i][keep], cols[keep]
        order = np.lexsort((ji, di))[:k]
        D[i, :order.size] = di[order]
        I[i, :order.size] = ji[order]
    return D, I


def knn_ref(oracle, x, c, k):
    """search(x, k) on the CPU, bit for bit: (D [n, k] float32, I [n, k] int64)."""
    dis, ok = distance_matrix(oracle, x, c)
    return select(dis, ok, k)
