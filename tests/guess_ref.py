"""Float64 models of the layer beneath the exact nearest-centroid search: the group means, the guess generators and
the per-tile group masks (csrc/prune.hip, at_filter_coarse and the second walk of assign_f16filter_kernel in
csrc/filter.hip, csrc/exact_search.cpp).  The exact search returns the dense sweep's bits whatever the guesses and the
masks are, so only a test that looks at them directly can tell a generator that searches the wrong groups, or a mask
with a wrong bit, from a correct one.  tests/test_guess_ref.py proves on the CPU that the inputs below give the GPU
tests (tests/test_gpu_guesses.py) something to prune and something to keep.  Built on off_origin_data.py (true_sqdist,
true_rowwise_sqdist, true_group_min, delta_bound).  TEST ONLY.

Contracts
    group means     means[g][f] = (fp32 sum of the live slots of group g in slot order) / float32(live slots); 0 for a
                    group of padding only.  The kernel's own arithmetic: compared bit for bit.
    guess mode      (group_only_mask_kernel) a 32-position tile searches exactly the groups its rows name, or the
                    union of gnbr[group] when a neighbour table is given: tile_candidates.
    coarse pass     (at_filter_coarse) a row's nearest group mean is found from the hi*hi product alone, so the mean
                    it names is any m with T_m <= min T + 2 eps_m, eps_m = filter_eps + filter_rho; the tile then
                    searches the union of gnbr[m] over its rows: coarse_sets brackets that set from below (rows with
                    one admissible mean) and from above (every admissible mean).
    prune masks     (prune_mask_kernel and the fused pre-pass of assign_f16filter_kernel) bit (tile, g) is set iff some
                    row of the tile has no guess or dmin[p][g] <= tau, tau = 2 sqrt(bd + 1.01 (2d + 8) 2^-24 (|x|^2 +
                    max|c|^2)): mask_bracket decides every pair that is not within `margin` of the threshold.
"""
import numpy as np

import off_origin_data as od

U = od.U
MARGIN = 1e-4          # the kernel's float32 tau against the float64 one: sqrtf, two multiplications and the
#                        (2d + 3)-term fmaf chain of |x|^2 inside delta, under 1e-5 relative in all; ten times that
NSUPER = 40

# ---- inputs ----------------------------------------------------------------------------------------------------------
GROUPS = {33: 2, 1285: 41, 2085: 66, 16384: 512}      # k -> ng (second group of one live slot / two mask words / a
#                                                       second 64-group pass with a 2-group tail / the size limit)
NS = (33, 127, 128, 129, 2033)                        # coarse: 128 (d = 64) or 64 (d = 128) rows per workgroup;
#                                                       pre-pass: 64 positions per wave, two tiles
BAND_RUNGS = ("origin", "db")                         # rungs on which `must` has to set 20 % .. 80 % of the pairs


def rung_params(name, d):
    return od.RUNGS[d][name]


def two_level(seed, n, k, d, offset, scale, nsuper=NSUPER):
    """(x [n, d], c [k, d]) float32: 40 super-centres from N(0, 1), centroids 0.15 N around a random super-centre, rows
    0.03 N around a random centroid, the table = those centres + 0.005 N jitter; everything moved by `offset` (a
    number, or "db" for a per-feature offset from U(-80, 0)) and scaled by `scale`.  Plain Gaussian centres are useless
    here: in d = 64 every wrong centroid is about 11 away and one near-miss guess per tile needs every group."""
    rng = np.random.default_rng(seed)
    sup = rng.standard_normal((nsuper, d))
    cen = sup[rng.integers(0, nsuper, k)] + 0.15 * rng.standard_normal((k, d))
    x = cen[rng.integers(0, k, n)] + 0.03 * rng.standard_normal((n, d))
    c = cen + 0.005 * rng.standard_normal((k, d))
    off = rng.uniform(-80.0, 0.0, d) if isinstance(offset, str) else np.full(d, float(offset))
    return (off + scale * x).astype(np.float32), (off + scale * c).astype(np.float32)


N_MAX = 2033
_DATA, _TRUTH = {}, {}


def table(name, d, k, seed=5, nsuper=NSUPER):
    """(x [2033, d], c [k, d]) of one rung of the two-level data, cached and read-only.  Every test at n < 2033 takes
    the first n rows, so that one table, one grouping and one float64 reference serve every n."""
    key = (name, d, k, seed, nsuper)
    if key not in _DATA:
        A, s = rung_params(name, d)
        x, c = two_level(seed, N_MAX, k, d, A, s, nsuper)
        x.setflags(write=False)
        c.setflags(write=False)
        _DATA[key] = (x, c)
    return _DATA[key]


def truth(name, d, k, seed=5, nsuper=NSUPER):
    """T [2033, k] float64 true squared distances of table(...), computed once (at most one table of 16384 centroids
    is kept: 266 MB each)."""
    key = (name, d, k, seed, nsuper)
    if key not in _TRUTH:
        if k > 4096:
            for old in [q for q in _TRUTH if q[2] > 4096]:
                del _TRUTH[old]
        x, c = table(*key)
        T = od.true_sqdist(x, c)
        T.setflags(write=False)
        _TRUTH[key] = T
    return _TRUTH[key]


# the pre-pass masks: (n, k); 16384 / 512 on `far` only -- on origin and db its tiles need 18 % of the groups, below
# the band that test_guess_ref.py holds every origin and db case to; 33 / 2 (one mask word with a 2-bit tail, the second
# group of one live slot) at n = 2033 only -- at n = 33 and 129 nearly every tile needs both groups (3-4 of 4 and 9-10
# of 10 pairs), which leaves no clear bit to get wrong
MASK_SHAPES = ((2033, 33), (33, 1285), (127, 1285), (128, 1285), (129, 1285), (2033, 1285), (129, 2085), (2033, 2085))
MASK_RUNGS = ("origin", "db", "far")
# (rung, d, n, k, none_tail): none_tail = None: every 37th row has no guess; 17: the rows without a guess start at
# position 2016 = 63 * 32, a tile boundary inside a wave; 97: at 1936 = 30 * 64 + 16, the middle of a wave's first tile
MASK_CASES = ([(r, d, n, k, None) for r in MASK_RUNGS for d in (64, 128) for (n, k) in MASK_SHAPES]
              + [("far", d, 2033, 16384, None) for d in (64, 128)]
              + [("origin", d, 2033, 1285, t) for d in (64, 128) for t in (17, 97)])
# the coarse pass, origin rung: (d, k) -> (seed, super-centres).  The walk over the group means keeps the hi*hi
# product only, so its eps is filter_eps + filter_rho and a super-centre that is split over several groups makes its
# rows ambiguous: the tables keep about 32 centroids per super-centre, and the seeds are those that hold the caps.
COARSE_TABLES = {(64, 33): (5, 40), (64, 1285): (5, 40), (64, 2085): (6, 66), (64, 16384): (5, 512),
                 (128, 33): (5, 40), (128, 1285): (8, 40), (128, 2085): (5, 65), (128, 16384): (6, 512)}
COARSE_CASES = [(d, n, k) for (d, k) in COARSE_TABLES for n in NS]
# the coarse pass on the hand-made grouping (kd_padded_cperm: 43 groups of 30 and a group of padding only, whose mean
# is the zero vector): (d, n, k) on table seed 6.  The last row is replaced by the zero row, the one row that names
# the zero mean; at n = 129 it is alone in its tile.
COARSE_PADDED_SEED = 6
COARSE_PADDED_CASES = [(d, n, 1285) for d in (64, 128) for n in (129, 2033)]


def coarse_padded_inputs(d, n, k):
    """(key, x [n, d] with row n - 1 zeroed, c, T [n, k]) of one COARSE_PADDED_CASES entry."""
    key = ("origin", d, k, COARSE_PADDED_SEED, NSUPER)
    x, c = table(*key)
    x = np.array(x[:n])
    x[n - 1] = 0.0
    T = np.array(truth(*key)[:n])
    T[n - 1] = sq_norms(c)
    return key, x, c, T


def kd_padded_cperm(cperm, holes=(3, 17)):
    """A hand-made grouping whose groups each carry padding slots in the middle: the rows of `cperm` (a kd grouping, so
    neighbours stay together) dealt 30 to a group with the slots `holes` left at -1, then one group of padding only."""
    rows = np.asarray(cperm)[np.asarray(cperm) >= 0]
    live = 32 - len(holes)
    ng = (rows.size + live - 1) // live
    out = np.full((ng + 1, 32), -1, np.int32)
    slots = [s for s in range(32) if s not in holes]
    for g in range(ng):
        part = rows[g * live:(g + 1) * live]
        out[g, slots[:part.size]] = part
    return out.reshape(-1)


def group_of(cperm, k):
    """[k] group of every centroid."""
    cp = np.asarray(cperm)
    out = np.full(k, -1, np.int64)
    out[cp[cp >= 0]] = np.nonzero(cp >= 0)[0] // 32
    return out


def group_neighbours_model(means, nnb):
    """uint32 [ng, ceil(ng/32)]: for every group the nnb groups with the nearest means in float64, itself first, ties to
    the lower index (at_group_neighbours_f32 scores in fp32: the two may differ where two means are equally far)."""
    means = np.asarray(means, np.float64)
    ng = means.shape[0]
    D = od.true_sqdist(means, means)
    out = np.zeros((ng, ng), bool)
    for g in range(ng):
        key = D[g].copy()
        key[g] = -1.0
        out[g, np.argsort(key, kind="stable")[:min(nnb, ng)]] = True
    return bool_to_bits(out)


def guesses(T, second_share=0.1, every=37, none_tail=None, seed=3):
    """ids int64 [n], dis float32 [n]: the float64 winner of every row; a share of the rows (chosen at random) guess their
    second-nearest centroid instead, so that tiles hold several runs and radii that reach other groups; every
    `every`-th row, or the last `none_tail` rows, have no guess (-1).  dis = the true squared distance to the guess."""
    n, k = T.shape
    rng = np.random.default_rng(seed)
    part = np.argpartition(T, min(1, k - 1), axis=1)[:, :2]
    first = T.argmin(axis=1)
    second = np.where(part[:, 0] == first, part[:, 1], part[:, 0])
    ids = np.where(rng.random(n) < second_share, second, first).astype(np.int64)
    dis = T[np.arange(n), ids].astype(np.float32)
    if none_tail is None:
        none = np.arange(n) % every == every - 1 if every else np.zeros(n, bool)
    else:
        none = np.arange(n) >= n - none_tail
    ids[none] = -1
    dis[none] = 0.0
    return ids, dis


def visit_order_model(ids, dis, k, dbits=8):
    """(order int64 [n], hint_sorted int64 [n]) as at_visit_order_f32 sorts: key = guess (k without one) << dbits |
    min(sqrt(max(dis, 0)) * (top / 2), top) truncated, top = 2^dbits - 1, float32 arithmetic; stable."""
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < k)
    top = np.float32((1 << dbits) - 1)
    if dis is None:
        r = np.zeros(ids.size, np.float32)
    else:
        r = np.sqrt(np.maximum(np.asarray(dis, np.float32), np.float32(0))) * (np.float32(0.5) * top)
    r = np.minimum(r, top).astype(np.uint32).astype(np.int64)
    key = (np.where(ok, ids, k) << dbits) | r
    order = np.argsort(key, kind="stable")
    return order, key[order] >> dbits


# ---- bit tables --------------------------------------------------------------------------------------------------------
def bits_to_bool(words, ng):
    """[rows, ceil(ng/32)] uint32 bit patterns (any 32-bit dtype) -> bool [rows, ceil(ng/32) * 32]: EVERY bit of every
    word, so that bits at or beyond ng show."""
    w = np.ascontiguousarray(words).view(np.uint32).reshape(len(words), -1)
    assert w.shape[1] == (ng + 31) // 32
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(w.shape[0], -1)


def bool_to_bits(b):
    """bool [rows, ng] -> uint32 [rows, ceil(ng/32)]."""
    rows, ng = b.shape
    full = np.zeros((rows, (ng + 31) // 32 * 32), np.uint64)
    full[:, :ng] = b
    return (full.reshape(rows, -1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def _per_tile_any(rows_bool):
    n = rows_bool.shape[0]
    ntile = (n + 31) // 32
    full = np.zeros((ntile * 32,) + rows_bool.shape[1:], bool)
    full[:n] = rows_bool
    return full.reshape((ntile, 32) + rows_bool.shape[1:]).any(axis=1)


# ---- models ------------------------------------------------------------------------------------------------------------
def group_means_model(c, cperm):
    """[ng, d] float32, the kernel's arithmetic: fp32 sum over the 32 slots in slot order, skipping -1, divided by
    float32(count); 0 for a group of padding only."""
    c = np.asarray(c, np.float32)
    cp = np.asarray(cperm).reshape(-1, 32)
    s = np.zeros((cp.shape[0], c.shape[1]), np.float32)
    cnt = np.zeros(cp.shape[0], np.int64)
    for m in range(32):
        live = cp[:, m] >= 0
        s[live] = s[live] + c[cp[live, m]]
        cnt += live
    out = np.zeros_like(s)
    some = cnt > 0
    out[some] = s[some] / cnt[some].astype(np.float32)[:, None]
    return out


def tile_candidates(groups_sorted, gnbr_or_none, ng):
    """bool [tiles, ng]: per 32-position tile the union over its rows of the row's group, or of gnbr[group] (uint32
    bit table [ng, ceil(ng/32)]) when a neighbour table is given.  A row that names no group (>= ng) adds nothing."""
    g = np.asarray(groups_sorted, np.int64)
    named = g < ng
    table = np.eye(ng, dtype=bool) if gnbr_or_none is None else bits_to_bool(gnbr_or_none, ng)[:, :ng]
    rows = np.zeros((g.size, ng), bool)
    rows[named] = table[g[named]]
    return _per_tile_any(rows)


def coarse_sets(x, means, gnbr, eps_m):
    """(L, U, admissible): per row the admissible nearest means {m : T_m <= min T + 2 eps_m} (bool [n, ng]); per tile
    of 32 consecutive rows L = union of gnbr[m] over the rows with exactly one admissible mean, U = union of gnbr[m]
    over every admissible mean of every row (bool [tiles, ng])."""
    T = od.true_sqdist(x, means)
    ng = means.shape[0]
    adm = T <= (T.min(axis=1) + 2.0 * np.asarray(eps_m, np.float64))[:, None]
    nb = bits_to_bool(gnbr, ng)[:, :ng]
    upper_rows = (adm.astype(np.float32) @ nb.astype(np.float32)) > 0
    single = adm.sum(axis=1) == 1
    lower_rows = np.zeros_like(upper_rows)
    lower_rows[single] = nb[T.argmin(axis=1)[single]]
    return _per_tile_any(lower_rows), _per_tile_any(upper_rows), adm


def mask_bracket(bd, p, has, dmin, xn, cnmax, d, margin=MARGIN):
    """(must, may) bool [tiles, ng] from the kernel's formula tau = 2 sqrt(bd + 1.01 (2d + 8) 2^-24 (xn + cnmax)):
    must[tile, g] when some row of the tile has no guess or dmin[p, g] <= tau (1 - margin); may: the same with
    (1 + margin).  bd, p, has, xn are per visiting position; dmin is [k, ng]."""
    bd, xn = np.asarray(bd, np.float64), np.asarray(xn, np.float64)
    has = np.asarray(has, bool)
    pc = np.where(has, np.asarray(p, np.int64), 0)
    with np.errstate(invalid="ignore"):
        tau = 2.0 * np.sqrt(np.where(has, bd, 0.0) + 1.01 * (2 * d + 8) * U * (xn + float(cnmax)))
    row = np.asarray(dmin, np.float64)[pc]
    must = row <= (tau * (1.0 - margin))[:, None]
    may = row <= (tau * (1.0 + margin))[:, None]
    must[~has] = True
    may[~has] = True
    return _per_tile_any(must), _per_tile_any(may)


def mask_brute(bd, p, has, dmin, xn, cnmax, d, factor):
    """mask_bracket's one side by plain loops (tiny cases only)."""
    n, ng = len(bd), dmin.shape[1]
    out = np.zeros(((n + 31) // 32, ng), bool)
    for i in range(n):
        for g in range(ng):
            if not has[i]:
                out[i // 32, g] = True
            else:
                tau = 2.0 * np.sqrt(float(bd[i]) + 1.01 * (2 * d + 8) * U * (float(xn[i]) + float(cnmax)))
                if float(dmin[p[i], g]) <= tau * factor:
                    out[i // 32, g] = True
    return out


def group_min_rows(c, cperm, rows):
    """od.true_group_min for the centroids `rows` only ([len(rows), ng] float64): what a table of 16384 centroids
    allows (the full matrix would be 2 GiB)."""
    cp = np.asarray(cperm).reshape(-1, 32)
    cc = np.sqrt(od.true_sqdist(np.asarray(c)[rows], c))
    cc = np.concatenate([cc, np.full((cc.shape[0], 1), np.inf)], axis=1)
    return cc[:, np.where(cp >= 0, cp, c.shape[0])].min(axis=2)


# ---- the a-priori bounds of csrc/filter.hip ---------------------------------------------------------------------------------
def filter_eps(d, H):
    """The a-priori bound of csrc/filter.hip on |P16 + |x|^2 - true squared distance| (header there)."""
    u, q, m = 2.0 ** -24, np.sqrt(d) * 2.0 ** -25, 3.0 * d / 16.0
    return H * (34 * m * u * 1.01 + 3 * 2.0 ** -22 + d * u * 1.01 + 2 * u + 2 * q) + 4 * q


def filter_rho(d, H):
    """filter_rho of csrc/filter.hip: the bound on |P(three products) - P(hi*hi only)|."""
    u, q, m = 2.0 ** -24, np.sqrt(d) * 2.0 ** -25, 2.0 * d / 16.0
    return H * ((2.0 ** -10 * 1.001 + 34.0 * m * u * 1.01 + 4.0 * u + q) * 1.0001) + 2.0 * q * 1.0001


def dmin_f16_bound(d, cp_sq, cmax_sq, three=False):
    """What at_group_min_dist_f16 subtracts from the squared distance: eps_a (1.001 |c_p|^2 + max|c|^2) + eps_b with
    the constants of at_group_min_dist_f16 / filter_tau / filter_rho (hi*hi form unless `three`)."""
    u, q, m = 2.0 ** -24, np.sqrt(d) * 2.0 ** -25, 3.0 * d / 16.0
    eps_h = 34.0 * m * u * 1.01 + 3.0 * 2.0 ** -22 + d * u * 1.01 + 2.0 * u + 2.0 * q
    delta_h = (2.0 * d + 8.0) * u * 1.01
    ta = (2.0 * delta_h + 2.0 * eps_h) * 1.0001
    tb = 8.0 * q * 1.0001
    ra = 0.0 if three else (2.0 ** -10 * 1.001 + 34.0 * (2.0 * d / 16.0) * u * 1.01 + 4.0 * u + q) * 1.0001
    rb = 0.0 if three else 2.0 * q * 1.0001
    eps_a = 0.5 * (ta - 2.0 * (2.0 * d + 8.0) * u * 1.01) * 1.001 + ra
    eps_b = 0.5 * tb * 1.001 + rb
    return eps_a * (1.001 * np.asarray(cp_sq, np.float64) + cmax_sq) + eps_b


def sq_norms(a):
    a = np.asarray(a, np.float64)
    return (a * a).sum(axis=1)


# ---- the inputs of one pre-pass case, shared by test_guess_ref.py and test_gpu_guesses.py --------------------------------
def mask_inputs(name, d, n, k, none_tail=None):
    """dict(x, c, T, ids, dis, order, hs, has): the first n rows of table(name, d, k), their guesses (guesses()) and
    the visiting order of those guesses (visit_order_model), hs = the guesses in visiting order (k = none)."""
    x, c = table(name, d, k)
    T = truth(name, d, k)[:n]
    ids, dis = guesses(T, none_tail=none_tail)
    order, hs = visit_order_model(ids, dis, k)
    return {"x": x[:n], "c": c, "T": T, "ids": ids, "dis": dis, "order": order, "hs": hs, "has": hs < k}


def coarse_eps(d, x, c):
    """(eps [n], eps_m [n]): filter_eps of every row against the table, and the eps of the walk over the group means
    (hi*hi only: filter_eps + filter_rho; the means' norms are below max|c|^2 by convexity)."""
    H = sq_norms(x) + sq_norms(c).max()
    return filter_eps(d, H), filter_eps(d, H) + filter_rho(d, H)
