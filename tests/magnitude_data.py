"""Unit-magnitude clusters moved to the ends of the fp32 range: the rungs of tests/test_magnitude_ref.py and
tests/test_gpu_magnitude.py.

Every other test of the exact nearest-centroid routes feeds them rows and centroids of magnitude 1.  Here the same
table (unit-normalised centroids with exact duplicates, rows near centroids and rows exactly on them, as
tests/test_gpu_knn.py builds it) is scaled by powers of two -- exactly, so a rung's answer is known from the control
wherever nothing under- or overflows -- and seeded with rows and centroids whose squares, norms or distances are
subnormal, vanish, or overflow to +inf from finite elements.

    unit      the control
    big       x 2^60: nothing overflows, every value is outside the fp16 range
    small     x 2^-40: nothing is subnormal, every value is below the fp16 range
    sub       x 2^-64: norms and distances are subnormal (~3e-39), squares of single elements lose bits
    zero      x 2^-80: every square, norm and product underflows; every distance is +0, every answer (0, +0.0)
    mixed     rows at unit scale; the centroids j % 4 == 1 x 2^-80 (distinct, but all of norm^2 0: every one of them is
              at distance |x|^2 exactly, the lowest index wins among them); 32 centroids x 2^62
    edge      x 2^63, with an antipodal plant: 32 centroids a_i close to one direction, 64 centroids m_j close to
              -1.05 times that direction (in groups of their own under group_rows_kd), 96 rows close to -0.8 times it.
              dis(x, a_i) ~ 2.8e38 and dis(x, m_j) ~ 5e36 are finite while the fp32 sum |m_j - a_i|^2 is +inf.
              edge_tiles: the same rows with the plants in rows 32 .. 127 (three whole 32-row tiles)
    unlisted  unit data plus rows whose |x|^2 is +inf from finite elements (one element 2e19; 64 elements of 2.4e18),
              rows of norm^2 ~1.4e38 whose xn + cn overflows only for the 16 centroids of norm^2 2.5e38, and 16
              centroids whose own norm^2 is +inf; the special rows sit first and last in a tile, fill whole tiles, and
              one is the lone row of the last tile

test_magnitude_ref.py proves these properties with the oracle alone.  TEST ONLY."""
import numpy as np
import torch

N = 4129                     # 129 tiles of 32 rows + one row
KS = (1000, 2080)            # ng = 32 with a padded last group; ng = 65
DS = (64, 128)
RUNG_NAMES = ("unit", "big", "small", "sub", "zero", "mixed", "edge", "edge_tiles", "unlisted")
EXP = {"unit": 0, "big": 60, "small": -40, "sub": -64, "zero": -80, "edge": 63, "edge_tiles": 63}
SHRINK, GROW = -80, 62       # mixed: the exponents of the shrunken and of the 32 grown centroids
N_A, N_M, N_PLANT = 32, 64, 96
INF = np.float32(np.inf)


def _unit(rng, n, d, oracle):
    return oracle.l2norm_rows(rng.standard_normal((n, d)).astype(np.float32))


def base(oracle, seed, n, d, k):
    """(x [n, d], c [k, d]) float32 as tests/test_gpu_knn.py::_data: unit-normalised centroids, 20 of them exact
    duplicates (k/2 ... k/2+19 repeat 0 ... 19); the first quarter of the rows 0.01 away from a centroid, 20 rows
    exactly on the duplicated centroids, the others anywhere on the sphere."""
    rng = np.random.default_rng(seed)
    c = _unit(rng, k, d, oracle)
    nd = min(20, k // 4)
    c[k // 2: k // 2 + nd] = c[0:nd]
    x = _unit(rng, n, d, oracle)
    q = n // 4
    x[:q] = (c[rng.integers(0, k, q)] + np.float32(0.01) * x[:q]).astype(np.float32)
    if q > nd:
        x[q: q + nd] = c[k // 2: k // 2 + nd]
    return x, c


def scale(a, e):
    """a * 2^e in float32 (exact wherever the result is a normal number)."""
    return np.ldexp(np.asarray(a, np.float32), e).astype(np.float32)


def rung(oracle, name, d, k, n=N, seed=9):
    """One rung: dict(x, c, e, and the index sets the rung's facts are about).  The same seed on every rung, so the
    same table at another magnitude.
        e           the rung's power of two (None on mixed and unlisted)
        shrunk, grown            mixed: centroid indices
        plant, a_ids, m_ids      edge: planted rows, their hints' pool, the far cluster
        plant_hint               edge: [n] int64, a_i for a planted row, -1 elsewhere
        overflow, edge_sum       unlisted: rows with |x|^2 = +inf; rows whose xn + cn overflows for `heavy` only
        heavy, infnorm           unlisted: the centroids of norm^2 2.5e38; those of norm^2 +inf"""
    x, c = base(oracle, seed, n, d, k)
    out = {"e": EXP.get(name)}
    if name in ("unit", "big", "small", "sub", "zero"):
        x, c = scale(x, EXP[name]), scale(c, EXP[name])
    elif name == "mixed":
        shrunk = np.arange(1, k, 4)
        grown = np.arange(2, 2 + 4 * 32, 4)
        c[shrunk] = scale(c[shrunk], SHRINK)
        c[grown] = scale(c[grown], GROW)
        out.update(shrunk=shrunk, grown=grown)
    elif name in ("edge", "edge_tiles"):
        rng = np.random.default_rng(seed + 1)
        # the common direction has positive components only, so group_rows_kd's power iteration (started from a
        # positive vector) finds +a and the far cluster, at the low end of every projection, fills whole groups
        a = np.abs(rng.standard_normal(d)) + 0.5
        a /= np.linalg.norm(a)
        spread = 0.01

        def near(m, f):
            v = a + spread * rng.standard_normal((m, d))
            return (f * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        a_ids = np.arange(40, 40 + N_A)
        m_ids = np.arange(k - 200, k - 200 + N_M)
        c[a_ids] = near(N_A, 1.0)
        c[m_ids] = near(N_M, -1.05)
        if name == "edge":
            plant = np.sort(np.random.default_rng(seed + 2).choice(np.arange(n // 4 + 32, n), N_PLANT, replace=False))
        else:
            plant = np.arange(32, 32 + N_PLANT)
        which = rng.integers(0, N_A, N_PLANT)
        x[plant] = (np.float32(-0.8) * c[a_ids[which]] + (0.8 * spread) * rng.standard_normal((N_PLANT, d))).astype(np.float32)
        hint = np.full(n, -1, np.int64)
        hint[plant] = a_ids[which]
        x, c = scale(x, EXP[name]), scale(c, EXP[name])
        out.update(plant=plant, a_ids=a_ids, m_ids=m_ids, plant_hint=hint)
    elif name == "unlisted":
        rng = np.random.default_rng(seed + 3)
        heavy = np.arange(200, 216)
        infnorm = np.arange(100, 116)
        sign = np.where(rng.random((16, d)) < 0.5, -1.0, 1.0)
        c[heavy] = (sign * np.sqrt(2.5e38 / d)).astype(np.float32)
        c[infnorm, 1] = np.float32(2e19)                     # (feature 1: the overflowing rows below use feature 0)
        # first and last of tile 0, tile 2 whole, mid-tile, the lone row of the last tile
        overflow = np.concatenate([[0, 31], np.arange(64, 96), [n // 3 + 5, n - 1]])
        edge_sum = np.concatenate([[32, 63], np.arange(96, 128), [n // 2 + 7]])
        w = min(64, d)
        for t, r in enumerate(overflow):
            if t % 2 == 0:
                x[r, 0] = np.float32(2e19)                   # one square overflows
            else:                                            # only the sum of w = 64 squares of 5.8e36 does
                x[r] = 0.0
                x[r, :w] = (np.where(rng.random(w) < 0.5, -1.0, 1.0) * np.sqrt(3.7e38 / w)).astype(np.float32)
        x[edge_sum] = (x[edge_sum] * np.float32(1.2e19)).astype(np.float32)
        out.update(overflow=overflow, edge_sum=edge_sum, heavy=heavy, infnorm=infnorm)
    else:
        raise KeyError(name)
    out.update(x=np.ascontiguousarray(x), c=np.ascontiguousarray(c))
    return out


def true_sqdist(a, b):
    """[na, nb] float64 squared distances, every one the float64 sum of the d squared float64 differences (never the
    expanded form): within (d + 2) 2^-53 relative of the truth; float64 has the range for every rung, squares of 2^-160
    and of 2^65 included."""
    ta = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    tb = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64))
    return (torch.cdist(ta, tb, p=2.0, compute_mode="donot_use_mm_for_euclid_dist") ** 2).numpy()


def true_group_min(c, cperm):
    """[k, ng] float64: min over the members m of group g of the true distance |c_p - c_m| (not squared); +inf for a
    group of padding only."""
    cp = np.asarray(cperm).reshape(-1, 32)
    cc = np.sqrt(true_sqdist(c, c))
    cc = np.concatenate([cc, np.full((cc.shape[0], 1), np.inf)], axis=1)
    return cc[:, np.where(cp >= 0, cp, c.shape[0])].min(axis=2)


def direct_sqdist_f32(a, b):
    """[na, nb] float32: the ascending fp32 fma chain over (a - b)^2, what a direct fp32 evaluation of |a - b|^2 gives
    (each step one rounding; emulated in float64, whose product and sum of two fp32-representable terms are exact
    before the rounding to float32 -- double rounding cannot turn a finite value into +inf or back here)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    with np.errstate(over="ignore"):
        for f in range(a.shape[1]):
            df = (a[:, None, f] - b[None, :, f]).astype(np.float64)
            acc = (df * df + acc.astype(np.float64)).astype(np.float32)
    return acc
