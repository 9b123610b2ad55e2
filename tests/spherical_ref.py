"""CPU reference of the inner-product search, the centroid re-normalisation and spherical k-means
(at_assign_ip_f32, at_renorm_rows_f32, ops.Kmeans(spherical=True)), numpy only.  TEST ONLY.

The contract: ip(i,j) is the fp32 fmaf chain over the feature index, ascending, from +0.  numpy
has no fmaf, so fma32 emulates one exactly: the product of two float32 values is exact in float64, the sum with c is
rounded ONCE to odd in float64 (TwoSum recovers what the addition lost), and 53 >= 24 + 2 bits make the final narrowing
to float32 the correctly rounded result of the exact a*b + c.  The plain "float64 multiply-add, then narrow" rounds
twice and is wrong on ties (tests/test_spherical_ref.py shows it); nothing here uses that shortcut."""
import numpy as np
import torch

import oracle
from centroid_sums_ref import finalize, sequential_sums
from oracle_backend import OracleBackend

_ONE = np.float32(1.0)


def fma32(a, b, c):
    """Exact float32 fmaf(a, b, c), elementwise with broadcasting."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)          # exact: 48 significant bits, exponent within range
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p                                               # TwoSum: s + err == p + c64 exactly
        err = (p - (s - bb)) + (c64 - bb)
        inexact = np.isfinite(s) & (err != 0)                    # (err is NaN where s is not finite)
        even = (s.view(np.int64) & 1) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(inexact & even, np.nextafter(s, toward), s)  # round to odd
        return s.astype(np.float32)


def fma32_naive(a, b, c):
    """The shortcut fma32 must not be: float64 multiply-add rounded to nearest, then narrowed (two roundings)."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def ip_matrix(x, c):
    """-> [n, k] float32: ip(i,j), d steps of fma32 from +0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    c = np.ascontiguousarray(c, dtype=np.float32)
    assert x.ndim == 2 and c.ndim == 2 and x.shape[1] == c.shape[1]
    acc = np.zeros((x.shape[0], c.shape[0]), np.float32)
    for f in range(x.shape[1]):
        acc = fma32(x[:, f:f + 1], c[None, :, f], acc)
    return acc


def search_ip_ref(x, c):
    """IndexFlatIP(c).search(x, 1) -> (ids int64 [n], ip float32 [n]): the lowest j with the largest product among
    the centroids with ip > -inf (a NaN product is never listed); nothing to list: (-1, -inf)."""
    ip = ip_matrix(x, c)
    n = ip.shape[0]
    with np.errstate(invalid="ignore"):
        listed = ip > -np.inf
    masked = np.where(listed, ip, -np.inf).astype(np.float32)
    ids = np.argmax(masked, axis=1).astype(np.int64)             # the first (lowest j) of the maxima
    best = ip[np.arange(n), ids] if n else np.zeros(0, np.float32)   # with its own bits
    none = ~listed.any(axis=1)
    ids[none] = -1
    best = np.where(none, np.float32(-np.inf), best).astype(np.float32)
    return ids, best


def renorm_ref(c):
    """faiss fvec_renorm_L2 per row -> a new array: nr = fma32 chain of c[f]^2; nr > 0: c * (1 / sqrt(nr)), every
    step rounded to float32; otherwise the row as it is."""
    c = np.ascontiguousarray(c, dtype=np.float32)
    nr = np.zeros(c.shape[0], np.float32)
    for f in range(c.shape[1]):
        nr = fma32(c[:, f], c[:, f], nr)
    out = c.copy()
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        go = nr > 0
        inv = (_ONE / np.sqrt(nr[go])).astype(np.float32)
        assert inv.dtype == np.float32
        out[go] = c[go] * inv[:, None]
    return out


class SphericalResult:
    __slots__ = ("centroids", "obj", "nsplit", "assign")


def spherical_kmeans_ref(x, k, niter, init=None, seed=1234):
    """faiss.Kmeans(d, k, niter=niter, spherical=True).train(x, init_centroids=init) as one straight-line loop."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, d = x.shape
    assert n >= k
    r = SphericalResult()
    r.obj, r.nsplit, r.assign = [], [], None
    if n > 256 * k:
        xs = x[oracle.rand_perm(n, seed)[:256 * k]]
    else:
        xs = x
    ns = xs.shape[0]
    if ns == k:                                   # faiss returns before any post-processing
        r.centroids, r.obj, r.nsplit = xs.copy(), [0.0], [0]
        return r
    cent = np.array(init, dtype=np.float32) if init is not None else xs[oracle.rand_perm(ns, seed + 1)[:k]]
    assert cent.shape == (k, d)
    cent = renorm_ref(cent)
    for _ in range(niter):
        ids, best = search_ip_ref(xs, cent)
        r.obj.append(float(np.float32(best.astype(np.float64).sum())))
        sums, counts, _, _ = sequential_sums(xs, ids, k)
        cent, hassign = finalize(sums[None], counts[None])
        nsplit = 0
        if (hassign == 0).any():
            nsplit, hassign, cent = oracle.split_clusters(hassign, cent, ns)
        r.nsplit.append(int(nsplit))
        cent = renorm_ref(cent)
        r.assign = ids
    r.centroids = cent
    return r


class SphericalOracleBackend(OracleBackend):
    """OracleBackend with the two methods ops.Kmeans(spherical=True) needs, from the reference above."""

    def assign_ip(self, x, c, want_dist=True):
        ids, ip = search_ip_ref(self._f32(x).numpy(), self._f32(c).numpy())
        return torch.from_numpy(ids), (torch.from_numpy(ip) if want_dist else None)

    def renorm_rows(self, c):
        assert c.dtype == torch.float32 and c.is_contiguous()
        c.copy_(torch.from_numpy(renorm_ref(c.numpy())))
        return c
