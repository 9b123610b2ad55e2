"""CPU reference of the asymmetric-distance search over product-quantiser codes (ops.IndexPQ.search, at_pq_search_f32).
TEST ONLY, no float64 anywhere.

The table T[i, m, j] comes from oracle.assign(x_m[at most 19 rows], cb[m][j:j+1]): the oracle's direct form (df = x - c,
acc = fmaf(df, df, acc) from +0, ascending), one codebook word at a time, as tests/knn_ref.py asks it per column.  The
distance of query i to database row r is T[i, 0, codes[r, 0]] + T[i, 1, codes[r, 1]] + ..., numpy float32 gathers added
in ascending m; knn_ref.select lists the k smallest (dis, r) with dis < +inf.  A row with a code >= ksub is masked out."""
import numpy as np

from knn_ref import select

DIRECT_ROWS = 19   # oracle.assign takes the direct form for calls of fewer than 20 rows


def pq_tables(oracle, x, codebooks):
    """T [n, M, ksub] float32.  Where the oracle lists nothing (the distance is NaN or not below +inf) the entry is
    whatever it reports, made unlistable: NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    cb = np.ascontiguousarray(codebooks, dtype=np.float32)
    n, d = x.shape
    M, ksub, dsub = cb.shape
    assert M * dsub == d
    T = np.empty((n, M, ksub), np.float32)
    for m in range(M):
        xm = np.ascontiguousarray(x[:, m * dsub:(m + 1) * dsub])
        for j in range(ksub):
            for i0 in range(0, n, DIRECT_ROWS):
                ids, dis = oracle.assign(xm[i0:i0 + DIRECT_ROWS], cb[m][j:j + 1])
                T[i0:i0 + DIRECT_ROWS, m, j] = np.where(ids == 0, dis, np.float32(np.nan))
    return T


def pq_distances(T, codes):
    """(dis [n, ntotal] float32, ok [n, ntotal] bool) from the tables and uint8 codes [ntotal, M]."""
    n, M, ksub = T.shape
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, M)
    ntotal = codes.shape[0]
    inside = (codes < ksub).all(1) if ntotal else np.zeros(0, bool)
    idx = np.minimum(codes.astype(np.int64), ksub - 1)
    dis = np.zeros((n, ntotal), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for m in range(M):
            term = T[:, m, :][:, idx[:, m]]
            dis = term.copy() if m == 0 else (dis + term).astype(np.float32)
    ok = np.broadcast_to(inside, (n, ntotal)) & (dis < np.float32(np.inf))
    return dis, ok


def pq_search_ref(oracle, x, codebooks, codes, k, tables=None):
    """(D [n, k] float32, I [n, k] int64): IndexPQ.search(x, k) on the CPU, bit for bit."""
    T = pq_tables(oracle, x, codebooks) if tables is None else tables
    dis, ok = pq_distances(T, codes)
    return select(dis, ok, k)
