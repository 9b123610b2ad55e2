"""Bit-exact reference of ops.IndexIVFPQ / at_ivfpq_search_f32, composed from what the suite already trusts.  TEST ONLY,
no float64 anywhere.

    lists / probes:  ivf_ref.ivf_lists / ivf_probes (knn_ref over the centroids)
    query of a (query, list) pair:  x[i] - c[l] in numpy float32, one subtraction per feature (by_residual), else x[i]
    tables, distances:  pq_search_ref.pq_tables / pq_distances on those queries and the code rows of the list
    row i:  ivf_ref.ivf_select -- the mask "row is in a probed list, list >= 0" and knn_ref.select.
The cost is M * ksub * ceil(pairs / 19) oracle calls: `probes` restricts the (query, list) pairs that are computed."""
import numpy as np

from ivf_ref import ivf_probes, ivf_select
from pq_search_ref import pq_distances, pq_tables


def ivfpq_encoder_input(x, lists, centroids, by_residual):
    """What the encoder sees of every stored row: x - c[list] (by_residual) or x; a zero vector for list -1."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    lists = np.asarray(lists, np.int64)
    out = x.copy()
    if by_residual:
        with np.errstate(over="ignore", invalid="ignore"):
            out = (x - np.asarray(centroids, np.float32)[np.maximum(lists, 0)]).astype(np.float32)
    out[lists < 0] = 0
    return out


def ivfpq_distances(oracle, x, codebooks, codes, lists, centroids, by_residual, probes=None):
    """(dis [n, ntotal] float32, ok [n, ntotal] bool): dis(i, r) for every stored row r of a list l >= 0 and every query i
    (with probes [n, nprobe]: only the queries that probe l; the other entries are not ok)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    codes = np.asarray(codes, np.uint8)
    lists = np.asarray(lists, np.int64)
    n, ntotal = x.shape[0], codes.shape[0]
    if not by_residual:
        dis, ok = pq_distances(pq_tables(oracle, x, codebooks), codes)
        return dis, ok & (lists >= 0)[None, :]
    cent = np.ascontiguousarray(centroids, dtype=np.float32)
    dis = np.full((n, ntotal), np.nan, np.float32)
    ok = np.zeros((n, ntotal), bool)
    for l in range(cent.shape[0]):
        rows = np.flatnonzero(lists == l)
        qs = np.arange(n) if probes is None else np.flatnonzero((np.asarray(probes) == l).any(1))
        if rows.size == 0 or qs.size == 0:
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            q = (x[qs] - cent[l][None, :]).astype(np.float32)
        dl, okl = pq_distances(pq_tables(oracle, q, codebooks), codes[rows])
        dis[np.ix_(qs, rows)] = dl
        ok[np.ix_(qs, rows)] = okl
    return dis, ok


def ivfpq_search_ref(oracle, x, codebooks, codes, lists, centroids, nprobe, k, by_residual, distances=None, probes=None):
    """IndexIVFPQ.search(x, k) on the CPU, bit for bit: (D [n, k] float32, I [n, k] int64).  distances: ivfpq_distances
    of (at least) the probed pairs, if at hand; probes: the probed lists, if not the quantiser's own."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    codes = np.asarray(codes, np.uint8)
    if x.shape[0] == 0 or codes.shape[0] == 0:
        return np.full((x.shape[0], k), np.inf, np.float32), np.full((x.shape[0], k), -1, np.int64)
    if probes is None:
        probes = ivf_probes(oracle, x, centroids, nprobe)
    dis, ok = distances if distances is not None else ivfpq_distances(oracle, x, codebooks, codes, lists, centroids,
                                                                      by_residual, probes=probes)
    return ivf_select(dis, ok, lists, probes, k)
