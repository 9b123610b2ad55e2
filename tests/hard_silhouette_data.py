"""Hard data for at_silhouette_f32: the rungs of tests/test_hard_silhouette_ref.py and tests/test_gpu_hard_silhouette.py.
Host only, numpy only.  rung(name) -> (x float32 [n, d], labels int64 [n]), built from a seed fixed by the name;
facts(name) -> what was planted.

Why bits can be demanded.  The recipe (tests/silhouette_ref.py) leaves one freedom, the order of the fp64 dot products
and norms.
  * Grid rows.  If every element of x is an integer multiple of one power of two q and 4 d (max |x| / q)^2 < 2^53, every
    fp64 product, partial dot, norm and ((-2 dot) + n_i) + n_j is an integer multiple of q^2 below 2^53 q^2: exact in
    any order (fused or not).  grid() asserts the bound.  A scaling of the whole sample by 2^e keeps that, as long as
    nothing leaves the fp32 normal range of x or the fp64 range of the products: grid() asserts this too.
  * d = 1.  One product per dot: nothing to reorder, for any values.
On such rows the reference, sklearn and a correct kernel have to agree in every bit.

    grid_d     (off, d): elements (off + integers) / 8, off = 0 and 2^20 (element offset 2^20 / 8), n = 300, 5 .. 9
               labels, d at and around the 64-dimension slab
    seams      (d, n, variant): cluster boundaries, in label-sorted order, at 31, 32, 33, 255, 256, 257 where n allows,
               one cluster filling the chunk [64, 96), one covering the query block [512, 768), singletons at both ends;
               variants k2 (two labels) and kmax (n - 1 labels, the pair across position 31 | 32); rows shuffled
    labels     one grid sample under labels 0 .. 4, under {INT64_MIN, -1, 0, 1, INT64_MAX} and under 2^40-spaced values
    order      d = 1: A = {0, -2^42}, B = 4096 rows at 1 with 2^54 and 2^30, C = 3 rows at 2^56.  S[0, B] in fp64 is
               2^54 + 2^30 + 4096 if the ones are added first (above the fp32 tie: rounds up) and 2^54 + 2^30 if they
               come last (each 1 is a quarter ulp of 2^54 and is lost; the tie rounds to even, down).
               "ones_first", "large_first", and "mixed": ones_first with A, B, C interleaved in row order
    offorigin  off = 2^20: clusters of identical rows, duplicates across clusters, a singleton on a member of another
    huge, overflow, tiny70, tiny76, vanish   one d = 7 grid (integers in [-64, 64) / 8, unclustered) x 2^58, 2^60, 2^-70,
               2^-76, 2^-80
    far        the same x 2^40, one cluster displaced by 2^63 in every dimension: 7 x 2^126 > fp32's maximum, so every
               d2 between it and the rest is +inf, whatever the fp64 order; its own rows get b = inf, a finite: NaN -> 0
    cancel     not a grid: 1000 + centre + 0.7 normal, d = 64, n = 1500, 12 labels.  No identical rows: off the grid
               the dot and the norm of two equal rows may round differently in fp64 and leave a d2 of a few ulps of the
               norm, which through the square root is worth more than the tolerance (sklearn has the same artefact)

TEST ONLY."""
import functools
import zlib

import numpy as np

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
Q_EXP = -3                                # q = 1 / 8
OFF = 1 << 20                             # in units of q: an element offset of 2^20 / 8
GRID_D_DIMS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
SEAM_N = (3, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1025)
SEAM_CUTS = (1, 31, 32, 33, 64, 96, 255, 256, 257, 769)     # planted boundaries (sorted positions), where n allows
SCALE_EXP = {"huge": 58, "overflow": 60, "tiny70": -70, "tiny76": -76, "vanish": -80}
FAR_EXP, FAR_SHIFT, FAR_LABEL = 40, 2.0 ** 63, 2
N_ONES = 4096

GRID_D = tuple("grid_d-%d-%d" % (off, d) for off in (0, OFF) for d in GRID_D_DIMS)
SEAMS = tuple("seams-%d-%d-%s" % (d, n, v) for d in (3, 65) for n in SEAM_N for v in ("planted", "k2", "kmax")
              if not (n < 31 and v != "k2"))
LABELS = ("labels-plain", "labels-ends", "labels-wide")
ORDER = ("order-ones_first", "order-large_first", "order-mixed")
OFFORIGIN = ("offorigin",)
SCALED = tuple(SCALE_EXP)
# every rung on which the recipe has no freedom left: compared bit for bit
BITWISE = GRID_D + SEAMS + LABELS + ORDER + OFFORIGIN + SCALED + ("far",)
GRID = GRID_D + SEAMS + LABELS + OFFORIGIN + SCALED          # built by grid() alone: the exactness bound holds
ALL = BITWISE + ("cancel",)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def exactness(ints, d):
    """4 d (max |x| / q)^2: below 2^53 every fp64 quantity of the recipe is exact in any order."""
    return 4 * d * int(np.abs(ints).max()) ** 2


def grid(ints, scale_exp=0):
    """int64 [n, d] -> float32 rows ints x 2^(Q_EXP + scale_exp), after the checks of the order-free regime."""
    ints = np.asarray(ints, dtype=np.int64)
    n, d = ints.shape
    assert exactness(ints, d) < 2 ** 53, ("outside the order-free regime", d, int(np.abs(ints).max()))
    x = ints.astype(np.float32)
    assert np.array_equal(x.astype(np.int64), ints)                       # the integers are fp32 numbers
    x = np.ldexp(x, Q_EXP + scale_exp).astype(np.float32)
    low = np.abs(x[x != 0]).min() if np.any(x != 0) else 1.0
    assert np.isfinite(x).all() and low >= 2.0 ** -126                   # the scaling lost no bit of x
    assert abs(2 * (Q_EXP + scale_exp)) + 60 < 1000                      # nor does fp64 lose one of a product
    return np.ascontiguousarray(x)


def _labels_all_present(rng, n, k):
    lab = rng.integers(0, k, n)
    lab[:k] = np.arange(k)
    return lab.astype(np.int64)


def _clustered(rng, lab, d, off=0):
    """Integers off + centre[label] + noise, inside off + [-64, 64)."""
    cen = rng.integers(-40, 40, (int(lab.max()) + 1, d))
    return off + cen[lab] + rng.integers(-24, 24, (len(lab), d))


def _sizes_to_labels(sizes):
    return np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)


def seam_cuts(n, variant):
    """The boundaries (first sorted position of every cluster but the first) of a seams rung."""
    if variant == "k2":
        return [1]                                                        # a singleton, then one cluster over all blocks
    if variant == "kmax":
        pair = 31 if n > 33 else n - 2                                    # positions pair, pair + 1 share a label
        return [p for p in range(1, n) if p != pair + 1]
    return sorted(set([c for c in SEAM_CUTS if c < n - 1] + [n - 1]))


@functools.lru_cache(maxsize=None)
def _build(name):
    rng = _rng(name)
    kind, _, rest = name.partition("-")
    fact = {}
    if kind == "grid_d":
        off, d = map(int, rest.split("-"))
        k = 5 + GRID_D_DIMS.index(d) % 5
        lab = _labels_all_present(rng, 300, k)
        x = grid(_clustered(rng, lab, d, off))
        fact.update(k=k)
    elif kind == "seams":
        d, n, variant = rest.split("-")
        d, n = int(d), int(n)
        cuts = seam_cuts(n, variant)
        sizes = np.diff([0] + cuts + [n])
        lab_sorted = _sizes_to_labels(sizes)
        ints = _clustered(rng, lab_sorted, d)
        perm = rng.permutation(n)                                         # row order != sorted order
        x, lab = grid(ints[perm]), lab_sorted[perm]
        fact.update(cuts=cuts, singletons=np.flatnonzero(np.bincount(lab)[lab] == 1))
    elif kind == "labels":
        base = _labels_all_present(_rng("labels"), 300, 5)
        x = grid(_clustered(_rng("labels-x"), base, 65, OFF))
        values = {"plain": [0, 1, 2, 3, 4], "ends": [I64_MIN, -1, 0, 1, I64_MAX],
                  "wide": [3 * 2 ** 40 + 5, -2 * 2 ** 40 + 5, 5, 2 ** 40 + 5, -2 ** 40 + 5]}[rest]
        lab = np.array(values, dtype=np.int64)[base]
    elif kind == "order":
        ones = np.ones(N_ONES)
        A, C = [0.0, -2.0 ** 42], [2.0 ** 56] * 3
        B = np.concatenate([[2.0 ** 54, 2.0 ** 30], ones] if rest == "large_first" else [ones, [2.0 ** 54, 2.0 ** 30]])
        x = np.concatenate([A, B, C]).astype(np.float32).reshape(-1, 1)
        lab = np.concatenate([np.zeros(2), np.ones(len(B)), np.full(3, 2)]).astype(np.int64)
        if rest == "mixed":
            # row 0 stays; the rest is dealt out so that A, B and C interleave, each keeping its own ascending order
            slot = np.sort(rng.permutation(np.arange(1, len(x)))[:4])     # where A's second row and C's rows go
            order = np.empty(len(x), np.int64)
            order[0] = 0
            rest_rows = np.setdiff1d(np.arange(1, len(x)), slot)
            order[slot] = [1, len(x) - 3, len(x) - 2, len(x) - 1]
            order[rest_rows] = np.arange(2, 2 + len(B))
            x, lab = x[order], lab[order]
        x = np.ascontiguousarray(x)
    elif kind == "offorigin":
        n, d, k = 300, 65, 7
        lab = _labels_all_present(rng, n, k)
        lab[lab == 6] = 5
        lab[299] = 6                                                      # label 6: a singleton
        ints = _clustered(rng, lab, d, OFF)
        same = np.flatnonzero(lab == 3)
        ints[same] = ints[same[0]]                                        # a cluster of identical rows: a = 0, s = 1
        dup_a, dup_b = np.flatnonzero(lab == 0)[:6], np.flatnonzero(lab == 1)[:6]
        ints[dup_a] = ints[dup_b]                                         # distance 0 across clusters, not the diagonal
        ints[299] = ints[np.flatnonzero(lab == 4)[0]]                     # the singleton sits on a member of cluster 4
        x = grid(ints)
        fact.update(same=same, dup=(dup_a, dup_b), singletons=np.array([299]))
    elif kind in SCALE_EXP or kind == "far":
        base = _rng("scaled")
        lab = _labels_all_present(base, 300, 5)
        ints = base.integers(-64, 64, (300, 7))
        if kind == "far":
            x = grid(ints, FAR_EXP)
            rows = np.flatnonzero(lab == FAR_LABEL)
            x[rows] = (x[rows] + np.float32(FAR_SHIFT)).astype(np.float32)
            assert np.isfinite(x).all() and 7 * FAR_SHIFT ** 2 * 0.99 > float(np.finfo(np.float32).max)
            fact.update(displaced=rows)
        else:
            x = grid(ints, SCALE_EXP[kind])
    elif kind == "cancel":
        n, d, k = 1500, 64, 12
        lab = _labels_all_present(rng, n, k)
        cen = rng.normal(size=(k, d))
        x = np.ascontiguousarray((1000.0 + cen[lab] + 0.7 * rng.normal(size=(n, d))).astype(np.float32))
        assert len(np.unique(x, axis=0)) == n
    else:
        raise KeyError(name)
    assert x.dtype == np.float32 and x.flags.c_contiguous and lab.dtype == np.int64 and len(x) <= 4500
    x.setflags(write=False)
    lab.setflags(write=False)
    return x, lab, fact


def rung(name):
    x, lab, _ = _build(name)
    return x, lab


def facts(name):
    return _build(name)[2]


def grid_ints(name):
    """The integers of a grid rung (x / q before the scaling), recovered exactly -> int64 [n, d]."""
    x, _ = rung(name)
    e = SCALE_EXP.get(name, 0)
    return np.ldexp(x.astype(np.float64), -(Q_EXP + e)).astype(np.int64)
