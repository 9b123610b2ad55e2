"""The magnitude rungs (tests/magnitude_data.py) are what they claim to be -- the oracle and the host helpers only, no GPU.

tests/test_gpu_magnitude.py holds every exact nearest-centroid route to the oracle on these rungs; that proves
something only if the rungs really reach the ends of the fp32 range they are named for.  At n = 4129, k in
(1000, 2080), d in (64, 128):

    big, small   the ids are the control's and every distance is the control's times 2^(2e), bit for bit
    sub          every row is listed; every distance is 0 or a subnormal number
    zero         every row is (0, +0.0)
    mixed        the rows that win at a shrunken centroid all name the lowest one, no row names a grown one
    edge         the planted rows win in the far cluster at a finite distance, their hints are at a finite distance above
                 2^126, and the fp32 direct |m - a_i|^2 is +inf for every member of the groups that hold the cluster
    unlisted     exactly the rows whose |x|^2 overflows are (-1, +inf); the rows whose xn + cn overflows for the heavy
                 centroids only are listed at a finite distance; nobody lists a centroid of infinite norm
    every rung   no distance is NaN

Measured (seed 9), the same for both k unless two figures are given:
    sub       subnormal winners 4109 of 4129 rows (0.995; the other 20 sit on their centroid at 0)
    mixed     rows at a shrunken centroid 0.805 / 0.804 (d = 64), 0.813 / 0.815 (d = 128); the others at a unit one
    edge      planted rows' distance at most 6.9e36 (d = 64), 8.3e36 (d = 128); to their hints 2.70e38 .. 2.82e38
              the far cluster fills groups 0 and 1 of group_rows_kd, which hold nothing else
    unlisted  36 rows at (-1, +inf); the 35 xn + cn rows all at centroid 0 and ~1.44e38 (every ordinary centroid ties
              there: 2 ip ~ 1e19 is below half an ulp of |x|^2)

group_rows_kd itself is held to two things here: a permutation whatever the table holds, and the same cuts at
every magnitude.  Before its coordinates were brought to magnitude 1 first, the 2^63 table gave NaN projections and
the call crashed in nth_element."""
import numpy as np
import pytest

import magnitude_data as md

_CACHE = {}
TINY = np.float32(2.0 ** -126)
CASES = [(d, k) for d in md.DS for k in md.KS]


@pytest.fixture(scope="module")
def helpers():
    from audio_tokens_amd.backend import HostHelpers
    return HostHelpers()


def _rung(oracle, name, d, k):
    """Computed once per (rung, d, k) and shared, never modified."""
    key = (name, d, k)
    if key not in _CACHE:
        r = md.rung(oracle, name, d, k)
        r["ids"], r["dis"] = oracle.assign(r["x"], r["c"])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = r
    return _CACHE[key]


def _pair_dist(oracle, x, c, rows, cols):
    """The contract's dis(x[rows[t]], c[cols[t]]) for every t (one oracle call per distinct column)."""
    out = np.empty(len(rows), np.float32)
    for j in np.unique(cols):
        sel = np.nonzero(cols == j)[0]
        pad = np.concatenate([x[rows[sel]], np.repeat(x[rows[sel[:1]]], 20, 0)])    # n >= 20: the expanded form
        out[sel] = oracle.assign(pad, c[j:j + 1])[1][:sel.size]
    return out


@pytest.mark.parametrize("name", md.RUNG_NAMES)
@pytest.mark.parametrize("d,k", CASES)
def test_shapes_and_no_nan(oracle, name, d, k):
    r = _rung(oracle, name, d, k)
    assert r["x"].shape == (md.N, d) and r["c"].shape == (k, d)
    assert r["x"].dtype == np.float32 and r["c"].dtype == np.float32
    assert np.isfinite(r["x"]).all() and np.isfinite(r["c"]).all()          # every overflow comes from finite input
    assert not np.isnan(r["dis"]).any()
    assert ((r["ids"] >= 0) == (r["dis"] < md.INF)).all()


@pytest.mark.parametrize("name", ["big", "small"])
@pytest.mark.parametrize("d,k", CASES)
def test_exact_scalings_of_the_control(oracle, name, d, k):
    u, r = _rung(oracle, "unit", d, k), _rung(oracle, name, d, k)
    e = r["e"]
    assert np.array_equal(r["x"], np.ldexp(u["x"], e)) and np.array_equal(r["c"], np.ldexp(u["c"], e))
    assert np.array_equal(r["ids"], u["ids"])
    assert np.array_equal(r["dis"].view(np.uint32), np.ldexp(u["dis"], 2 * e).astype(np.float32).view(np.uint32))
    if name == "big":        # outside the fp16 range: the filter has to hand every row to the fp32 sweep
        assert (np.abs(r["c"]).max(axis=1) > 65504.0).all() and (np.abs(r["x"]).max(axis=1) > 65504.0).all()
    else:                    # below the smallest fp16 subnormal: every fp16 image is 0
        assert np.abs(r["c"]).max() < 2.0 ** -25 and np.abs(r["x"]).max() < 2.0 ** -25
        nz = r["dis"][r["dis"] > 0]
        assert nz.min() >= TINY


@pytest.mark.parametrize("d,k", CASES)
def test_sub_is_subnormal(oracle, d, k):
    r = _rung(oracle, "sub", d, k)
    ids, dis = r["ids"], r["dis"]
    assert (ids >= 0).all()
    assert ((dis == 0) | ((dis > 0) & (dis < TINY))).all()
    share = float(((dis > 0) & (dis < TINY)).mean())
    print(f"\nMEASURE sub d={d} k={k}: subnormal winners {share:.4f}")
    assert share >= 0.9
    xn = np.einsum("ij,ij->i", r["x"].astype(np.float64), r["x"].astype(np.float64))
    assert xn.max() < 2.0 ** -126                                            # the norms themselves are subnormal
    sq = (r["c"][:8].astype(np.float64) ** 2)
    assert (sq.astype(np.float32) != sq).any()                               # single squares lose bits


@pytest.mark.parametrize("d,k", CASES)
def test_zero_is_zero(oracle, d, k):
    r = _rung(oracle, "zero", d, k)
    assert (r["x"] != 0).any(axis=1).all() and (r["c"] != 0).any(axis=1).all()     # the data are not zero ...
    assert (r["ids"] == 0).all() and (r["dis"].view(np.uint32) == 0).all()         # ... every distance is +0


@pytest.mark.parametrize("d,k", CASES)
def test_mixed_classes(oracle, d, k):
    r = _rung(oracle, "mixed", d, k)
    ids = r["ids"]
    shrunk, grown = r["shrunk"], r["grown"]
    assert shrunk.size >= k // 4 - 1 and grown.size == 32
    assert np.unique(r["c"][shrunk], axis=0).shape[0] == np.unique(_rung(oracle, "unit", d, k)["c"][shrunk], axis=0).shape[0]
    cn = np.array([oracle.assign(np.zeros((20, d), np.float32), r["c"][j:j + 1])[1][0] for j in shrunk[:40]])
    assert (cn.view(np.uint32) == 0).all()                                   # norm^2 +0
    at_shrunk = np.isin(ids, shrunk)
    assert (ids[at_shrunk] == shrunk.min()).all()
    assert not np.isin(ids, grown).any()
    share = float(at_shrunk.mean())
    print(f"\nMEASURE mixed d={d} k={k}: rows at a shrunken centroid {share:.4f}, at a unit one {1 - share:.4f}")
    assert share >= 0.05 and 1.0 - share >= 0.05


@pytest.mark.parametrize("name", ["edge", "edge_tiles"])
@pytest.mark.parametrize("d,k", CASES)
def test_edge_plant(oracle, helpers, name, d, k):
    r = _rung(oracle, name, d, k)
    x, c, ids, dis, plant = r["x"], r["c"], r["ids"], r["dis"], r["plant"]
    assert plant.size == md.N_PLANT >= 64
    if name == "edge_tiles":
        assert np.array_equal(plant, np.arange(32, 128))
    else:
        assert np.unique(plant // 32).size > 32                              # scattered over the tiles
    assert np.isin(ids[plant], r["m_ids"]).all() and np.isfinite(dis[plant]).all()
    hint = r["plant_hint"][plant]
    assert np.isin(hint, r["a_ids"]).all() and (r["plant_hint"][np.setdiff1d(np.arange(md.N), plant)] == -1).all()
    dh = _pair_dist(oracle, x, c, plant, hint)
    print(f"\nMEASURE {name} d={d} k={k}: planted rows' distance max {dis[plant].max():.3g}, to their hints "
          f"{dh.min():.4g} .. {dh.max():.4g}")
    assert np.isfinite(dh).all() and (dh > np.float32(2.0 ** 126)).all()
    rest = np.setdiff1d(np.arange(md.N), plant)
    assert (ids[rest] >= 0).all() and np.isfinite(dis[rest]).all()
    # the grouping keeps the far cluster in groups of its own, and from every a_i each of their members overflows
    cperm = helpers.group_rows_kd(c)
    assert np.array_equal(np.sort(cperm[cperm >= 0]), np.arange(k))
    cp = cperm.reshape(-1, 32)
    groups = np.unique(np.nonzero(np.isin(cp, r["m_ids"]))[0])
    members = cp[groups].ravel()
    members = members[members >= 0]
    assert np.array_equal(np.sort(members), r["m_ids"]), "the far cluster shares a group with other centroids"
    direct = md.direct_sqdist_f32(c[r["a_ids"]], c[members])
    assert np.isposinf(direct).all()
    true = md.true_sqdist(c[r["a_ids"]], c[members])
    assert np.isfinite(true).all() and true.max() < 4.0 * float(dh.astype(np.float64).min())   # |m - a_i| < 2 |x - a_i|: Elkan cannot skip them
    # the cuts do not depend on the magnitude
    assert np.array_equal(cperm, helpers.group_rows_kd(md.scale(c, -r["e"])))


@pytest.mark.parametrize("d,k", CASES)
def test_unlisted_rows(oracle, d, k):
    r = _rung(oracle, "unlisted", d, k)
    x, c, ids, dis = r["x"], r["c"], r["ids"], r["dis"]
    ov, es = r["overflow"], r["edge_sum"]
    assert np.array_equal(np.nonzero(ids < 0)[0], np.sort(ov)) and np.isposinf(dis[ov]).all()
    x64 = x.astype(np.float64)
    assert ((x64[ov[0::2]] ** 2).max(axis=1) > 3.5e38).all()                 # one square overflows
    assert ((x64[ov[1::2]] ** 2).max(axis=1) < 1e37).all() and ((x64[ov[1::2]] ** 2).sum(axis=1) > 3.5e38).all()
    assert (ids[es] >= 0).all() and np.isfinite(dis[es]).all()
    xn = (x64[es] ** 2).sum(axis=1)
    cn = (c.astype(np.float64) ** 2).sum(axis=1)
    assert (xn < 3e38).all() and (xn + cn[r["heavy"]].min() > 3.5e38).all()
    assert np.array_equal(np.nonzero(cn > 3.5e38)[0], r["infnorm"])
    assert not np.isin(ids, r["infnorm"]).any() and not np.isin(ids, r["heavy"]).any()
    for j in (r["heavy"][0], r["infnorm"][0]):                               # and they are at +inf from the xn + cn rows
        assert np.isposinf(_pair_dist(oracle, x, c, es, np.full(es.size, j))).all()
    # first and last in a tile, a whole tile, the lone last row
    for rows in (ov, es):
        pos = set((rows % 32).tolist())
        assert 0 in pos and 31 in pos
        assert any(np.isin(np.arange(t * 32, t * 32 + 32), rows).all() for t in range(4))
    assert md.N - 1 in ov


@pytest.mark.parametrize("what", ["unlisted", "nan", "inf", "huge", "tiny"])
def test_grouping_is_a_permutation_whatever_the_table_holds(oracle, helpers, what):
    k, d = 1000, 64
    c = md.rung(oracle, "unlisted" if what == "unlisted" else "unit", d, k)["c"].copy()
    if what == "nan":
        c[7, 3] = np.nan
    elif what == "inf":
        c[7, 3], c[9, 0] = np.inf, -np.inf
    elif what == "huge":
        c = md.scale(c, 127)
    elif what == "tiny":
        c = md.scale(c, -140)
    cperm = helpers.group_rows_kd(c)
    assert cperm.size == 32 * 32 and np.array_equal(np.sort(cperm[cperm >= 0]), np.arange(k))
    assert ((cperm.reshape(-1, 32) >= 0).sum(axis=1)[:-1] == 32).all()


@pytest.mark.parametrize("e", [-100, -30, 30, 63, 100])
def test_grouping_cuts_do_not_depend_on_the_magnitude(oracle, helpers, e):
    """A table scaled by 2^e, well inside the normal range with all its sums, is cut exactly as the unit one."""
    for d, k in ((64, 1000), (128, 2080)):
        c = md.rung(oracle, "unit", d, k)["c"]
        assert np.array_equal(helpers.group_rows_kd(md.scale(c, e)), helpers.group_rows_kd(c)), (d, k)


@pytest.mark.parametrize("d", md.DS)
def test_the_objective_at_2_50_stays_finite(oracle, d):
    """tests/test_gpu_magnitude.py trains on 2 x 8192 rows x 2^50 (k = 1024, 4 iterations): squared distances ~2^101, the
    fp32 objective of 8192 rows ~2^114 -- below 2^128, so the oracle can be compared on it."""
    import warnings
    x = md.scale(md.base(oracle, 9, 2 * 8192, d, 1024)[0], 50)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r1 = oracle.kmeans_train(x[:8192], 1024, niter=4)
        r2 = oracle.kmeans_train(x[8192:], 1024, niter=4, init_centroids=r1.centroids)
    for r in (r1, r2):
        assert r.obj.dtype == np.float32 and np.isfinite(r.obj).all() and (r.obj > 2.0 ** 100).all()
        assert np.isfinite(r.centroids).all()
