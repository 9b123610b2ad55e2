"""Clustered data with a common offset: the ladder of tests/test_off_origin_ref.py and tests/test_gpu_off_origin.py.

Every other test of the exact nearest-centroid routes feeds them data centred on the origin, where |x|^2 + |c|^2 is of
the order of the distances and the rounding term delta = (2d + 8) u (|x|^2 + max|c|^2) of the fp32 contract is
negligible.  Here every feature carries an offset A and the clusters have spread s, so |x|^2 + |c|^2 ~ 2 d A^2 while
the distances are ~ d s^2: the further down the ladder, the more of a computed distance is rounding noise.

    origin  (0, 1)       the same clusters at the origin: the control
    far     (100, 0.8 at d = 64, 1.2 at d = 128)   delta is felt, the Elkan rule still skips nearly everything
    edge    (100, 0.6 at d = 64, 0.8 at d = 128)   the inflated radius reaches most centroids: pruning fades out
    clamp   (100, 0.2)   a fifth to a quarter of the rows compute a negative distance and clamp to 0
    wrong   (100, 0.1)   half the rows at 0; the contract's winner is no longer the fp64 winner for some percent
    flat    (100, 0.01)  every row at 0 with hundreds of centroids tied there: the lowest index decides everything
    db      per-feature offset U(-80, 0), s = 10: raw log-mel in dB; the offset is large, the spread is too

test_off_origin_ref.py proves these properties with the oracle and float64 alone.  TEST ONLY."""
import numpy as np
import torch

N, K = 4129, 1000            # 129 tiles of 32 rows + one row; ng = 32 groups, the last one padded

RUNGS = {
    64: {"origin": (0.0, 1.0), "far": (100.0, 0.8), "edge": (100.0, 0.6), "clamp": (100.0, 0.2),
         "wrong": (100.0, 0.1), "flat": (100.0, 0.01), "db": ("db", 10.0)},
    128: {"origin": (0.0, 1.0), "far": (100.0, 1.2), "edge": (100.0, 0.8), "clamp": (100.0, 0.2),
          "wrong": (100.0, 0.1), "flat": (100.0, 0.01), "db": ("db", 10.0)},
}
RUNG_NAMES = ("origin", "far", "edge", "clamp", "wrong", "flat", "db")
U = 2.0 ** -24


def build(seed, n, k, d, A, s):
    """(x [n, d], c [k, d]) float32: k Gaussian cluster centres scaled by s and moved by the offset A (a number, or
    "db" for a per-feature offset drawn from U(-80, 0)); rows 0.3 s around a random centre, centroids 0.05 s around
    theirs; 20 duplicated centroids (k/2 ... k/2+19 repeat 0 ... 19) with a row on each."""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((k, d))
    off = rng.uniform(-80.0, 0.0, d) if isinstance(A, str) else np.full(d, float(A))
    x = off + s * (cen[rng.integers(0, k, n)] + 0.3 * rng.standard_normal((n, d)))
    c = off + s * (cen + 0.05 * rng.standard_normal((k, d)))
    c[k // 2: k // 2 + 20] = c[0:20]
    x[:20] = c[k // 2: k // 2 + 20]
    return x.astype(np.float32), c.astype(np.float32)


def rung(name, d, seed=9, n=N, k=K):
    """One rung of the ladder: the same seed on every rung, so the same clusters, rows and duplicates at another
    offset and spread."""
    A, s = RUNGS[d][name]
    return build(seed, n, k, d, A, s)


def delta_bound(x, c):
    """[n] float64: (2d + 8) u (|x|^2 + max|c|^2), the bound of csrc/prune.hip on |computed - true| squared distance."""
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return (2 * x.shape[1] + 8) * U * ((x64 ** 2).sum(1) + (c64 ** 2).sum(1).max())


def true_sqdist(a, b):
    """[na, nb] float64 squared distances, every one the float64 sum of the d squared float64 differences (never the
    expanded form |a|^2 + |b|^2 - 2 a.b, which cancels exactly where these data are hard): within (d + 2) 2^-53
    relative of the truth.  (The square of cdist's root adds three roundings to the d + 1 of the sum.)"""
    ta = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    tb = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64))
    return (torch.cdist(ta, tb, p=2.0, compute_mode="donot_use_mm_for_euclid_dist") ** 2).numpy()


def true_rowwise_sqdist(a, b):
    """[n] float64: |a_i - b_i|^2 from differences."""
    diff = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return (diff * diff).sum(1)


def true_group_min(c, cperm):
    """[k, ng] float64: min over the members m of group g of the true distance |c_p - c_m| (not squared); +inf for a
    group of padding only.  cperm: int array [ng * 32], -1 padded."""
    cp = np.asarray(cperm).reshape(-1, 32)
    cc = np.sqrt(true_sqdist(c, c))
    cc = np.concatenate([cc, np.full((cc.shape[0], 1), np.inf)], axis=1)     # column k: what a padding slot reads
    return cc[:, np.where(cp >= 0, cp, c.shape[0])].min(axis=2)


def facts(x, c, cperm=None):
    """The float64 truth a test needs: dict(T = squared distances [n, k], arg = arg-min [n] (lowest index on equal
    values), gmin = true_group_min(c, cperm) when a grouping is given)."""
    T = true_sqdist(x, c)
    out = {"T": T, "arg": T.argmin(axis=1)}
    if cperm is not None:
        out["gmin"] = true_group_min(c, cperm)
    return out
