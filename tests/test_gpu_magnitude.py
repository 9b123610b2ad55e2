"""Every exact nearest-centroid route at the ends of the fp32 range (tests/magnitude_data.py), bit for bit.

The accelerated routes promise the bits of the plain fp32 contract for ANY input, but every other test feeds them rows
and centroids of magnitude 1.  The shortcuts rest on real-number arguments that fp32 breaks at the ends of its range:
a distance of +inf ties with the +inf a running best starts from, a direct |c_p - c_m|^2 overflows where the
expanded form of the sweep is still finite, the relative error model delta = (2d + 8) u (|x|^2 + max|c|^2) has no
absolute term for subnormal sums, and a NaN threshold compares false with everything.  The rungs (proved on the CPU
by test_magnitude_ref.py): unit, big (x 2^60), small (x 2^-40), sub (x 2^-64), zero (x 2^-80), mixed (centroids x 2^-80
and x 2^62 among unit ones), edge / edge_tiles (x 2^63 with an antipodal plant), unlisted (rows without a finite
distance, centroids of infinite norm).

Shapes: n = 4129 (129 tiles of 32 + a tile of one row), k = 1000 (ng = 32, the last group padded) and k = 2080
(ng = 65), d = 64 and 128; the other dense forms at n = 1500, k = 300.  Every comparison is bit for bit against
oracle.assign, knn_ref or oracle.kmeans_train; the only other assertions are the float64 lower-bound property of dmin
and the two list conditions the fp16 range check implies.

The contract for rows without a finite distance ("Rows without a finite distance"): (-1, +inf) on every
route, whatever the hints were; a +inf distance never ties its way into an answer.

WHAT THE TESTS EXPOSED (each fixed with this file; with the fix taken out again the tests named fail)
  * Ties at +inf.  The exact update of the hinted and both pruned sweeps (assign.hip) and the reduction of the filter's
    per-row redo (exact_rows_body, filter.hip) accept a lower index on an equal distance, +inf included: the 36 rows
    of `unlisted` whose |x|^2 overflows came back as (0, +inf) instead of (-1, +inf), and from iteration 2 on
    Kmeans.train added them into a centroid (24 of 64 centroids wrong after 4 iterations on the hinted path, 4 of 1024
    on the pruned one).  assign.hip: test_dense_and_hinted_sweeps[unlisted-*], test_pruned_filtered_and_unguided_routes
    [unlisted-*] (filter=False), test_training_ignores_unlisted_rows[64-4129]; filter.hip: the same pruned test at
    filter=True and test_training_ignores_unlisted_rows[1024-8192].
  * dmin overflow read as "far".  group_min_dist_kernel's direct sum |c_p - c_m|^2 is +inf for the far cluster of
    `edge` seen from the a_i (128 bounds of +inf per table), `inf <= tau` is false and the winner's group was skipped:
    60-62 wrong ids of 4129 when the planted rows guess their a_i, 1-3 under random guesses.
    test_dmin_is_a_lower_bound[edge-*-0], test_pruned_filtered_and_unguided_routes[edge-*] and [edge_tiles-*].
  * A NaN radius skipped every group in prune_mask_kernel and read as "past n" in the pre-pass fused into the filter
    sweep: with either guard taken out a tile with a NaN row visited 648 of 1056 / 804 of 2145 (tile, group) pairs
    instead of all.  test_a_nan_radius_looks_everywhere (the separate kernel's count, then the fused one's).
  * group_rows_kd (host): the 2^63 table overflowed its fp32 covariance sums, the projections came out NaN and
    nth_element ran off its range -- a crash of the process.  tests/test_magnitude_ref.py::test_edge_plant and
    ::test_grouping_is_a_permutation_whatever_the_table_holds.
  * Nothing on: the dense sweeps in every form (MFMA at d = 64 / 128 and its variants 1 and 3, any-d at 80 and 640,
    the generic kernel, the unaligned branch, the direct form), knn and IndexFlatL2.search on every rung; big, small,
    sub, zero and mixed on every route; the subnormal error model (sub prunes like unit and keeps every bit); the
    trainings at 2^-64 and 2^50; rows with NaN / +-Inf elements on every route, the knn lists at 8 / 32 / 40, the index
    and the other dense forms included (nobody else harmed in ids or distance bits, the bad rows' ids in [-1, k)).

MEASURED on an MI355X (the MEASURE lines; records of which regime ran, not thresholds)

Rows the filter listed for the fp32 redo, of the rows it swept: unit 0.0305 (d = 64) / 0.0378 (d = 128) at k = 1000;
every other rung 1.0000 (big, edge, mixed, unlisted: outside the fp16 range; small, sub, zero: all gaps below the
absolute term of tau).

(tile, group) pairs the fp32 pre-pass kept, all rows, summed over the hint sets: every pair on unit, big, small, sub,
zero and unlisted (three quarters of the rows lie anywhere on the sphere, at distance ~1.2: twice that radius reaches
every group); mixed 0.982 under the fp32 bounds; edge 0.9955 (d = 64) / 0.9978 (d = 128).  The rows close to their
centroids swept alone, true guesses with distances, fp32 bounds, visited / total:
    rung                    d=64 k=1000   d=64 k=2080   d=128 k=1000   d=128 k=2080
    unit, big, small, sub   496 / 1056    693 / 2145    482 / 1056     679 / 2145     (identical on the four rungs)
    edge                    998 / 1056    1875 / 2145   961 / 1056     1675 / 2145
under the fp16 bounds (dmin_kernel 1, 2) everything is visited except on unit: they give 0 throughout outside the fp16
range and below it.

dmin: the fp32 kernel's mean bound / mean truth is 1.0000 on big, small and sub and 0.9907 on edge (0.037 of the
bounds are 0: the duplicated centroids and the overflowing pairs); never above the float64 truth.

Oracle repair counts of the trainings (cold / warm): sub d=64 [0, 0, 0, 0] / [287, 74, 4, 0], d=128 [0, 2, 0, 0] /
[572, 259, 47, 3]; 2^50 d=64 [0, 0, 0, 0] / [287, 86, 4, 0], d=128 [0, 3, 0, 0] / [572, 352, 128, 14]; objectives
~1.2e-35 and ~5e33.
"""
import warnings

import numpy as np
import pytest
import torch

import magnitude_data as md
from knn_ref import distance_matrix, select

pytestmark = pytest.mark.gpu

N = md.N
_REF, _GRP, _DMAT = {}, {}, {}
INF = np.float32(np.inf)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ref(oracle, name, d, k, n=N):
    """One rung with the oracle's answer (ids, dis): computed once, shared, read-only."""
    key = (name, d, k, n)
    if key not in _REF:
        if name == "big50" or name == "big60":
            r = md.rung(oracle, "unit", d, k, n=n)
            e = int(name[3:])
            r.update(x=md.scale(r["x"], e), c=md.scale(r["c"], e), e=e)
        else:
            r = md.rung(oracle, name, d, k, n=n)
        r["ids"], r["dis"] = oracle.assign(r["x"], r["c"])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _grouping(be, name, d, k, c):
    key = (name, d, k)
    if key not in _GRP:
        _GRP[key] = be.group_rows_kd(c)
    return _GRP[key]


def _same(got, r, what, want_dist=True, rows=None):
    ids, dis = got
    ids = ids.cpu().numpy()
    ids_o, dis_o = r["ids"], r["dis"]
    if rows is not None:
        ids, ids_o, dis_o = ids[rows], ids_o[rows], dis_o[rows]
    bad = np.nonzero(ids != ids_o)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {ids.size} ids differ, first at row {bad[0]}: got {ids[bad[0]]} want "
                           f"{ids_o[bad[0]]} (distance {dis_o[bad[0]]})")
    if want_dist:
        dg = dis.cpu().numpy()
        if rows is not None:
            dg = dg[rows]
        bad = np.nonzero(bits(dg) != bits(dis_o))[0]
        assert bad.size == 0, f"{what}: {bad.size} distances differ, first at row {bad[0]}: got {dg[bad[0]]!r} want {dis_o[bad[0]]!r}"
    else:
        assert dis is None, what


def _fp64_winner(x, c):
    """The float64 arg-min from the expanded form (a guess only: its own rounding does not matter)."""
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        T = (x64 * x64).sum(1)[:, None] + (c64 * c64).sum(1)[None, :] - 2.0 * (x64 @ c64.T)
    return np.argmin(np.nan_to_num(T, nan=np.inf), axis=1).astype(np.int64)


def _hints(be, rng, r, k):
    """name -> (per-row guesses int64, their distances or None)."""
    n = r["ids"].size
    dev = be.device
    truth = torch.from_numpy(r["ids"]).to(dev)
    dtruth = torch.from_numpy(r["dis"]).to(dev)
    out = {
        "truth": (truth, dtruth),
        "random": (torch.from_numpy(rng.integers(0, k, n)).to(dev), None),
        "none": (torch.full((n,), -1, dtype=torch.int64, device=dev), None),
        "fp64": (torch.from_numpy(_fp64_winner(r["x"], r["c"])).to(dev), None),
        "beyond_k": (torch.from_numpy(k + rng.integers(0, 7, n)).to(dev), None),
    }
    if "plant_hint" in r:          # edge: the planted rows guess their a_i, the others the truth
        h = np.where(r["plant_hint"] >= 0, r["plant_hint"], r["ids"])
        out["a_i"] = (torch.from_numpy(h).to(dev), None)
    if "infnorm" in r:             # unlisted: every row guesses a centroid of infinite norm
        out["infnorm"] = (torch.from_numpy(r["infnorm"][rng.integers(0, 16, n)].astype(np.int64)).to(dev), None)
    return out


def _settle(be, oracle, d):
    """A filtered call on the control: leaves the context in the asynchronous form."""
    r = _ref(oracle, "unit", d, 1000)
    xt, ct = be._f32(r["x"]), be._f32(r["c"])
    cperm = be.from_host(_grouping(be, "unit", d, 1000, r["c"]))
    dmin = be.group_min_dist(ct, cperm)
    order = be.visit_order(torch.from_numpy(r["ids"]).to(be.device), None, 1000)
    be.filter_stats()
    for _ in range(2):
        be.assign_pruned(xt, ct, order, cperm, dmin, filter=True)
        be.filter_stats()


@pytest.fixture()
def settled(request, be, oracle):
    """For tests that switch the filter's forms or train: once the test is through (and, asked for ahead of `switches`,
    once the switches are back at their defaults) a filtered call on the control leaves the context in the
    asynchronous form, whatever the test did and however it ended."""
    yield
    _settle(be, oracle, request.node.callspec.params.get("d", 64))


RUNG_CASES = [(name, d, k) for d in md.DS for k in md.KS for name in md.RUNG_NAMES]


# ---------------------------------------------------------------------------------------------------------------------
# the dense and the hinted sweep

@pytest.mark.parametrize("name,d,k", RUNG_CASES)
def test_dense_and_hinted_sweeps(be, oracle, name, d, k):
    """assign, and assign_hinted told the truth, random ids, nothing, the float64 winner and ids >= k (on edge also the
    antipodal a_i, on unlisted also a centroid of infinite norm), in row order and in member-list order, with and
    without distances."""
    r = _ref(oracle, name, d, k)
    xt, ct = be._f32(r["x"]), be._f32(r["c"])
    _same(be.assign(xt, ct), r, "assign")
    _same(be.assign(xt, ct, want_dist=False), r, "assign ids only", want_dist=False)
    for hname, (hint, _) in _hints(be, np.random.default_rng(d + k), r, k).items():
        hint = hint.contiguous()
        _, member_order = be.centroid_accum(xt, torch.clamp(hint, min=0, max=k - 1), k, want_order=True)
        for oname, order in (("row order", None), ("member-list order", member_order)):
            for want_dist in (True, False):
                _same(be.assign_hinted(xt, ct, hint, order, want_dist=want_dist), r,
                      f"assign_hinted hint={hname} {oname} want_dist={want_dist}", want_dist)


OTHER_RUNGS = ("sub", "zero", "mixed", "unlisted", "big60")


@pytest.mark.parametrize("name", OTHER_RUNGS)
@pytest.mark.parametrize("form", ["anyd80", "anyd640", "generic50", "unaligned80", "direct19", "variant1", "variant3"])
def test_other_dense_forms(be, oracle, switches, name, form):
    """k = 300, 1500 rows: the any-d chunked sweep (d = 80, 640), the generic kernel (d = 50), the scalar branch for rows
    that are not 16-byte aligned, the direct form for fewer than 20 rows, and the assign_variant 1 and 3 kernels."""
    from device_rows import rows_one_float_off
    d = {"anyd80": 80, "anyd640": 640, "generic50": 50, "unaligned80": 80, "direct19": 64, "variant1": 64, "variant3": 128}[form]
    r = _ref(oracle, name, d, 300, n=1500)
    if form == "direct19":                      # the first 19 rows: another formula, so another reference
        x = np.ascontiguousarray(r["x"][:19])
        ids_o, dis_o = oracle.assign(x, r["c"])
        assert not np.isnan(dis_o).any()
        r = {"ids": ids_o, "dis": dis_o, "c": r["c"]}
        xt = be._f32(x)
    elif form == "unaligned80":
        xt = rows_one_float_off(r["x"], be.device)
    else:
        xt = be._f32(r["x"])
    if form.startswith("variant"):
        switches(assign_variant=int(form[-1]))
    ct = be._f32(r["c"])
    _same(be.assign(xt, ct), r, f"assign {form}")
    _same(be.assign(xt, ct, want_dist=False), r, f"assign {form} ids only", want_dist=False)


# ---------------------------------------------------------------------------------------------------------------------
# the pruned sweep, the fp16-split filter and its finishing paths, the unguided searches

@pytest.mark.parametrize("name,d,k", RUNG_CASES)
def test_pruned_filtered_and_unguided_routes(be, oracle, settled, switches, name, d, k):
    """assign_pruned -- the fp32 sweep alone and behind the filter -- under each of the three centroid-to-group bound
    kernels, in the synchronous form, with the separate pre-pass and with the LDS-staged sweep, under every hint set;
    assign_c2f plain and coherent; assign_unguided with and without a grouping.  Two list conditions the fp16 range
    check implies: on `big` and on `unlisted` (whose heavy centroids lie outside the fp16 range) the filter hands every
    row, the overflowing ones included, to the fp32 redo."""
    r = _ref(oracle, name, d, k)
    xt, ct = be._f32(r["x"]), be._f32(r["c"])
    cperm = be.from_host(_grouping(be, name, d, k, r["c"]))
    hints = _hints(be, np.random.default_rng(d + k + 1), r, k)
    forms = [{"dmin_kernel": 0}, {"dmin_kernel": 1}, {"dmin_kernel": 2}, {"filter_sync": 1}, {"filter_fused": 0},
             {"filter_sync": 1, "filter_fused": 0}, {"prune_kernel": 0}, {"prune_kernel": 0, "dmin_kernel": 0}]
    counts = {}
    for form in forms:
        switches(dmin_kernel=1, filter_sync=0, filter_fused=1, prune_kernel=1)
        switches(**form)
        dmin = be.group_min_dist(ct, cperm)
        tag = ",".join(f"{a}={b}" for a, b in form.items())
        rows_seen = listed_seen = needed_seen = total_seen = 0
        for hname, (hint, hd) in hints.items():
            order = be.visit_order(hint.contiguous(), hd, k)
            flts = (True,) if ("filter_sync" in form or "filter_fused" in form) else (False, True)
            for flt in flts:
                for want_dist in (True, False):
                    be.filter_stats()
                    be.prune_stats(reset=True)
                    got = be.assign_pruned(xt, ct, order, cperm, dmin, want_dist=want_dist, filter=flt)
                    what = f"assign_pruned {name} hint={hname} filter={flt} want_dist={want_dist} [{tag}]"
                    _same(got, r, what, want_dist)
                    rows, listed = be.filter_stats()
                    assert rows == (N if flt else 0), what
                    rows_seen += rows
                    listed_seen += listed
                    if not flt:
                        needed, total = be.prune_stats()
                        needed_seen += needed
                        total_seen += total
                    if flt and name == "big":
                        assert listed == N, f"{what}: listed {listed} of {N}"
                    if flt and name == "unlisted":   # the heavy centroids put max |c|^2 outside the fp16 range: the sweep
                        assert listed == N, f"{what}: listed {listed} of {N}"   # lists every row, the overflowing ones among them
        counts[tag] = (listed_seen, rows_seen, needed_seen, total_seen)
    switches(dmin_kernel=1, filter_sync=0, filter_fused=1, prune_kernel=1)
    for tag, (listed, rows, needed, total) in counts.items():
        print(f"\nMEASURE {name} d={d} k={k} [{tag}]: listed {listed} of {rows} filtered rows ({listed / max(rows, 1):.4f})"
              + (f"; fp32 sweep visited {needed} of {total} (tile, group) pairs ({needed / total:.4f})" if total else ""))
    dmin = be.group_min_dist(ct, cperm)
    for want_dist in (True, False):
        _same(be.assign_c2f(xt, ct, cperm, dmin, want_dist=want_dist), r, "assign_c2f", want_dist)
        _same(be.assign_c2f(xt, ct, cperm, dmin, want_dist=want_dist, coherent=True), r, "assign_c2f coherent", want_dist)
        _same(be.assign_unguided(xt, ct, want_dist=want_dist), r, "assign_unguided", want_dist)
        _same(be.assign_unguided(xt, ct, want_dist=want_dist, cperm=cperm), r, "assign_unguided kd", want_dist)


@pytest.mark.parametrize("dk", [0, 1, 2])
@pytest.mark.parametrize("name,d,k", [(name, d, k) for d in md.DS for k in md.KS for name in ("big", "small", "sub", "edge")])
def test_dmin_is_a_lower_bound(be, oracle, switches, name, d, k, dk):
    """dmin[p][g] <= the true min over the members of group g of |c_p - c_m|, for every p and g, compared in float64
    against the float64 sum of d squared differences (within (d + 2) 2^-53 relative: hence the factor 1 + 1e-12 and
    nothing else).  Only a group of padding may read +inf -- on `edge` the fp32 sum |c_p - c_m|^2 itself is +inf for
    the far cluster seen from the a_i, and a bound of +inf there makes the sweep skip the winner's group."""
    switches(dmin_kernel=dk)
    r = _ref(oracle, name, d, k)
    c = r["c"]
    cperm = _grouping(be, name, d, k, c)
    gmin = md.true_group_min(c, cperm)
    assert np.isfinite(gmin).all()
    got = be.group_min_dist(be._f32(c), be.from_host(cperm)).cpu().numpy().astype(np.float64)
    assert got.shape == gmin.shape and not np.isnan(got).any()
    assert np.isfinite(got).all(), f"{np.isinf(got).sum()} bounds of +inf for groups that hold centroids"
    over = got > gmin * (1.0 + 1e-12)
    assert not over.any(), f"{over.sum()} bounds above the truth, worst by {(got - gmin)[over].max():.3e}"
    print(f"\nMEASURE dmin {name} d={d} k={k} dmin_kernel={dk}: bounds at 0: {(got == 0).mean():.3f}, "
          f"mean bound / mean truth {got.mean() / gmin.mean():.4f}")
    if k == 1000:      # a group of padding only behind the table: +inf there, the other columns unchanged -- or 0
        # throughout, where an fp16 kernel has given up on a table outside the fp16 range ("visit everything")
        padded = np.concatenate([cperm, np.full(32, -1, np.int32)])
        got2 = be.group_min_dist(be._f32(c), be.from_host(padded)).cpu().numpy()
        assert got2.shape == (k, gmin.shape[1] + 1)
        assert np.isposinf(got2[:, -1]).all() or (dk != 0 and (got2 == 0).all())
        assert np.array_equal(got2[:, :-1].astype(np.float64), got)


@pytest.mark.parametrize("name,d,k", [(name, d, k) for d in md.DS for k in md.KS for name in ("unit", "big", "small", "sub", "edge")])
def test_pruning_among_rows_close_to_their_centroids(be, oracle, settled, switches, name, d, k):
    """The rows of the table are mostly anywhere on the sphere, at distance ~1.2 from their winner: twice that radius
    reaches every group and the masks of the test above are full.  The first quarter of the rows lies 0.01 from a
    centroid; swept alone, with true guesses, their radius 2 sqrt(1e-4 + delta) ~ 0.02 is far below the spacing of the
    centroids (~1.4) and the masks really prune -- at `sub` with a delta that is a handful of subnormal ulps, on sums
    whose every fma step has an absolute error of half such an ulp.  The control must prune under the fp32 bounds."""
    r = _ref(oracle, name, d, k)
    q = N // 4
    near = {"ids": r["ids"][:q], "dis": r["dis"][:q]}
    xt, ct = be._f32(np.ascontiguousarray(r["x"][:q])), be._f32(r["c"])
    cperm = be.from_host(_grouping(be, name, d, k, r["c"]))
    truth, dtruth = torch.from_numpy(near["ids"]).to(be.device), torch.from_numpy(near["dis"]).to(be.device)
    for dk in (0, 1, 2):
        switches(dmin_kernel=dk)
        dmin = be.group_min_dist(ct, cperm)
        for hd in (dtruth, None):
            order = be.visit_order(truth, hd, k)
            for form in ({}, {"prune_kernel": 0}, {"filter_fused": 0}, {"filter_sync": 1}):
                switches(prune_kernel=1, filter_fused=1, filter_sync=0)
                switches(**form)
                for flt in (False, True):
                    be.filter_stats()
                    be.prune_stats(reset=True)
                    what = f"near rows {name} dmin_kernel={dk} distances={hd is not None} filter={flt} {form}"
                    _same(be.assign_pruned(xt, ct, order, cperm, dmin, filter=flt), near, what)
                    rows, listed = be.filter_stats()
                    needed, total = be.prune_stats()
                    if not form and hd is not None:
                        print(f"\nMEASURE near rows {name} d={d} k={k} dmin_kernel={dk} filter={flt}: listed {listed} of "
                              f"{rows}; visited {needed} of {total} (tile, group) pairs")
                    if name == "unit" and dk == 0 and not flt:
                        assert 0 < needed <= (3 * total) // 4, what     # (a tile's 32 rows name ~20 of 32 groups, ~25 of 65)
    switches(dmin_kernel=1, prune_kernel=1, filter_fused=1, filter_sync=0)


# ---------------------------------------------------------------------------------------------------------------------
# k nearest centroids

def _dmat(oracle, name, d):
    key = (name, d)
    if key not in _DMAT:
        r = _ref(oracle, name, d, 1000)
        D, ok = distance_matrix(oracle, r["x"], r["c"])
        assert not np.isnan(D).any()
        D.setflags(write=False)
        ok.setflags(write=False)
        _DMAT[key] = (D, ok)
    return _DMAT[key]


@pytest.mark.parametrize("d", md.DS)
@pytest.mark.parametrize("name", ["sub", "zero", "mixed", "unlisted", "edge"])
def test_knn_lists(be, oracle, name, d):
    """be.knn with k = 8 and 32 (the fused lists) and 40 (the general path) against knn_ref at k_c = 1000; column 0 is
    assign's answer on every row (no distance is NaN on these rungs), and IndexFlatL2.search(x, 1) and (x, 8) agree."""
    from audio_tokens_amd.ops import IndexFlatL2
    r = _ref(oracle, name, d, 1000)
    D, ok = _dmat(oracle, name, d)
    xt, ct = be._f32(r["x"]), be._f32(r["c"])
    for kk in (8, 32, 40):
        Dr, Ir = select(D, ok, kk)
        assert np.array_equal(Ir[:, 0], r["ids"]) and np.array_equal(bits(Dr[:, 0]), bits(r["dis"]))
        if name == "zero":
            assert (Ir == np.arange(kk)).all() and (bits(Dr) == 0).all()
        I, Dg = be.knn(xt, ct, kk)
        I, Dg = I.cpu().numpy(), Dg.cpu().numpy()
        assert np.array_equal(I, Ir), f"k={kk}: {(I != Ir).any(axis=1).sum()} of {N} lists differ"
        assert np.array_equal(bits(Dg), bits(Dr)), f"k={kk}"
        I2, none = be.knn(xt, ct, kk, want_dist=False)
        assert none is None and np.array_equal(I2.cpu().numpy(), Ir), f"k={kk} ids only"
    index = IndexFlatL2(d, backend=be)
    index.add(r["c"])
    for kk in (1, 8):
        Dr, Ir = select(D, ok, kk)
        Ds, Is = index.search(r["x"], kk)
        assert np.array_equal(np.asarray(Is), Ir), f"search k={kk}: {(np.asarray(Is) != Ir).any(axis=1).sum()} rows differ"
        assert np.array_equal(bits(np.asarray(Ds)), bits(Dr)), f"search k={kk}"


# ---------------------------------------------------------------------------------------------------------------------
# rows with a NaN or an infinite element keep their documented status: no defined winner, and no harm to the others

@pytest.mark.parametrize("d,k", [(64, 1000), (128, 2080)])
def test_bad_rows_harm_nobody(be, oracle, settled, switches, d, k):
    """Unit data with NaN, +inf and -inf elements in rows placed first, last and mid-tile (and in the lone row of the
    last tile): on every route every other row keeps the oracle's bits, and the bad rows' ids lie in [-1, k)."""
    r0 = _ref(oracle, "unit", d, k)
    x = r0["x"].copy()
    badrows = np.array([0, 31, 47, 64, 95, 2000, N - 1])
    for t, row in enumerate(badrows):
        x[row, (5 * t) % d] = (np.nan, np.inf, -np.inf)[t % 3]
    good = np.setdiff1d(np.arange(N), badrows)
    ids_o, dis_o = oracle.assign(x, r0["c"])
    assert np.array_equal(ids_o[good], r0["ids"][good]) and np.array_equal(bits(dis_o[good]), bits(r0["dis"][good]))
    r = {"ids": ids_o, "dis": dis_o}
    xt, ct = be._f32(x), be._f32(r0["c"])
    cperm = be.from_host(_grouping(be, "unit", d, k, r0["c"]))

    def check(got, what, want_dist=True):
        _same(got, r, what, want_dist, rows=good)
        b = got[0].cpu().numpy()[badrows]
        assert ((b >= -1) & (b < k)).all(), f"{what}: bad rows answer {b}"

    rng = np.random.default_rng(d)
    hints = {"truth": torch.from_numpy(np.where(ids_o < 0, 3, ids_o)).to(be.device),
             "random": torch.from_numpy(rng.integers(0, k, N)).to(be.device),
             "none": torch.full((N,), -1, dtype=torch.int64, device=be.device)}
    check(be.assign(xt, ct), "assign")
    for hname, hint in hints.items():
        _, member_order = be.centroid_accum(xt, torch.clamp(hint, min=0), k, want_order=True)
        for order in (None, member_order):
            check(be.assign_hinted(xt, ct, hint, order), f"assign_hinted {hname}")
    for form in ({}, {"dmin_kernel": 0}, {"filter_sync": 1}, {"filter_fused": 0}, {"prune_kernel": 0}):
        switches(dmin_kernel=1, filter_sync=0, filter_fused=1, prune_kernel=1)
        switches(**form)
        dmin = be.group_min_dist(ct, cperm)
        for hname, hint in hints.items():
            order = be.visit_order(hint.contiguous(), None, k)
            for flt in (False, True):
                for want_dist in (True, False):
                    check(be.assign_pruned(xt, ct, order, cperm, dmin, want_dist=want_dist, filter=flt),
                          f"assign_pruned {hname} filter={flt} {form}", want_dist)
    switches(dmin_kernel=1, filter_sync=0, filter_fused=1, prune_kernel=1)
    dmin = be.group_min_dist(ct, cperm)
    check(be.assign_c2f(xt, ct, cperm, dmin), "assign_c2f")
    check(be.assign_c2f(xt, ct, cperm, dmin, coherent=True), "assign_c2f coherent")
    check(be.assign_unguided(xt, ct), "assign_unguided")
    check(be.assign_unguided(xt, ct, cperm=cperm), "assign_unguided kd")
    # the k nearest lists and the index: the good rows' whole lists, ids and distance bits; the bad rows' ids in range
    from audio_tokens_amd.ops import IndexFlatL2
    D, ok = distance_matrix(oracle, x, r0["c"])

    def check_lists(I, Dg, kk, what):
        Dr, Ir = select(D, ok, kk)
        assert np.array_equal(Ir[good, 0], ids_o[good]), what
        I = np.asarray(I)
        bad = np.nonzero((I[good] != Ir[good]).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {bad.size} lists differ, first at row {good[bad[0]]}: {I[good[bad[0]]]} want {Ir[good[bad[0]]]}"
        if Dg is not None:
            assert np.array_equal(bits(np.asarray(Dg)[good]), bits(Dr[good])), f"{what}: distances differ"
        b = I[badrows]
        assert ((b >= -1) & (b < k)).all(), f"{what}: bad rows list {b}"

    for kk in (8, 32, 40):
        I, Dg = be.knn(xt, ct, kk)
        check_lists(I.cpu().numpy(), Dg.cpu().numpy(), kk, f"knn k={kk}")
        I2, none = be.knn(xt, ct, kk, want_dist=False)
        assert none is None
        check_lists(I2.cpu().numpy(), None, kk, f"knn k={kk} ids only")
    index = IndexFlatL2(d, backend=be)
    index.add(r0["c"])
    for kk in (1, 8):
        Ds, Is = index.search(x, kk)
        check_lists(Is, Ds, kk, f"IndexFlatL2.search k={kk}")


@pytest.mark.parametrize("form", ["anyd80", "anyd640", "generic50", "unaligned80", "direct19", "variant1", "variant3"])
def test_bad_rows_harm_nobody_in_the_other_dense_forms(be, oracle, switches, form):
    """The same bad rows (NaN, +inf, -inf elements; first, last and mid-tile, the last row) through the any-d sweep, the
    generic kernel, the unaligned branch, the direct form and the assign_variant 1 and 3 kernels, k = 300, 1500 rows."""
    from device_rows import rows_one_float_off
    d = {"anyd80": 80, "anyd640": 640, "generic50": 50, "unaligned80": 80, "direct19": 64, "variant1": 64, "variant3": 128}[form]
    r0 = _ref(oracle, "unit", d, 300, n=1500)
    n = 19 if form == "direct19" else 1500
    x = r0["x"][:n].copy()
    badrows = np.array([0, 7, 18]) if n == 19 else np.array([0, 31, 47, 64, 95, 700, n - 1])
    for t, row in enumerate(badrows):
        x[row, (5 * t) % d] = (np.nan, np.inf, -np.inf)[t % 3]
    good = np.setdiff1d(np.arange(n), badrows)
    ids_o, dis_o = oracle.assign(x, r0["c"])
    assert not np.isnan(dis_o[good]).any()
    r = {"ids": ids_o, "dis": dis_o}
    xt = rows_one_float_off(x, be.device) if form == "unaligned80" else be._f32(x)
    if form.startswith("variant"):
        switches(assign_variant=int(form[-1]))
    ct = be._f32(r0["c"])
    for want_dist in (True, False):
        got = be.assign(xt, ct, want_dist=want_dist)
        _same(got, r, f"assign {form}", want_dist, rows=good)
        b = got[0].cpu().numpy()[badrows]
        assert ((b >= -1) & (b < 300)).all(), f"assign {form}: bad rows answer {b}"


@pytest.mark.parametrize("d,k", [(64, 1000), (128, 2080)])
def test_a_nan_radius_looks_everywhere(be, oracle, settled, switches, d, k):
    """The rows close to their centroids, in row order with their true guesses, prune (the test above).  With a NaN
    element in one row of every 32-row tile, that row's radius 2 sqrt(bd + delta) is NaN, and `dmin <= NaN` is false
    for every group: the pre-pass -- the separate kernel and the one fused into the filter sweep -- has to read it as
    +inf, so every tile needs every group (prune_stats), and the other rows keep the oracle's bits."""
    switches(dmin_kernel=0)
    r = _ref(oracle, "unit", d, k)
    q = N // 4
    x = r["x"][:q].copy()
    bad = np.arange(5, q, 32)
    x[bad, 7] = np.nan
    good = np.setdiff1d(np.arange(q), bad)
    near = {"ids": r["ids"][:q], "dis": r["dis"][:q]}
    xt, ct = be._f32(x), be._f32(r["c"])
    cperm = be.from_host(_grouping(be, "unit", d, k, r["c"]))
    dmin = be.group_min_dist(ct, cperm)
    order = (torch.arange(q, dtype=torch.int32, device=be.device),
             torch.from_numpy(near["ids"].astype(np.int32)).to(be.device))
    be.prune_stats(reset=True)
    _same(be.assign_pruned(xt, ct, order, cperm, dmin, filter=False), near, "assign_pruned", rows=good)
    needed, total = be.prune_stats(reset=True)
    assert total == (cperm.numel() // 32) * ((q + 31) // 32)
    assert needed == total, f"visited {needed} of {total} (tile, group) pairs"
    for form in ({}, {"filter_fused": 0}, {"filter_sync": 1}):
        switches(filter_fused=1, filter_sync=0)
        switches(**form)
        _same(be.assign_pruned(xt, ct, order, cperm, dmin, filter=True), near, f"assign_pruned filter {form}", rows=good)
    # the pre-pass fused into the filter sweep keeps no masks; under filter_stats its (needed, total) arrive in
    # prune_stats: there a NaN radius also read as "position past n", and the row asked for nothing
    switches(filter_fused=1, filter_sync=0)
    _settle(be, oracle, d)
    switches(filter_stats=1)
    be.prune_stats(reset=True)
    _same(be.assign_pruned(xt, ct, order, cperm, dmin, filter=True), near, "assign_pruned fused, counted", rows=good)
    needed, total = be.prune_stats(reset=True)
    assert total == (cperm.numel() // 32) * ((q + 31) // 32)
    assert needed == total, f"fused pre-pass: visited {needed} of {total} (tile, group) pairs"
    switches(filter_stats=0)


# ---------------------------------------------------------------------------------------------------------------------
# training

@pytest.mark.parametrize("d", md.DS)
@pytest.mark.parametrize("name", ["sub", "big50"])
def test_training_at_both_ends(be, oracle, settled, name, d):
    """Kmeans(d, 1024, niter=4) on 8192 rows, then a warm start on another 8192 (both prune: n >= 4096, k >= 1024),
    pruned and dense: centroids and repair counts the oracle's bit for bit, objectives within the suite's rtol 2e-5.
    At 2^50 the squared distances are ~2^101 and the fp32 objective of 8192 rows ~2^114: finite."""
    from audio_tokens_amd.ops import Kmeans
    k, n1, niter = 1024, 8192, 4
    e = -64 if name == "sub" else 50
    x = md.scale(md.base(oracle, 9, 2 * n1, d, k)[0], e)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r1 = oracle.kmeans_train(x[:n1], k, niter=niter)
        r2 = oracle.kmeans_train(x[n1:], k, niter=niter, init_centroids=r1.centroids)
        assert np.isfinite(r1.obj).all() and np.isfinite(r2.obj).all() and (r1.obj > 0).all()
        print(f"\nMEASURE training {name} d={d}: oracle nsplit cold {list(r1.nsplit)} warm {list(r2.nsplit)}, "
              f"objective {r1.obj[-1]:.4g} / {r2.obj[-1]:.4g}")
        got = {}
        for prune in (True, False):
            km = Kmeans(d, k, niter=niter, backend=be)
            km.prune = prune
            km.train(x[:n1])
            cold = (km.centroids.copy(), list(km.obj), [st["nsplit"] for st in km.iteration_stats])
            km.train(x[n1:], init_centroids=km.centroids)
            got[prune] = cold + (km.centroids.copy(), list(km.obj), [st["nsplit"] for st in km.iteration_stats])
    for prune, a in got.items():
        what = f"prune={prune}"
        assert np.array_equal(bits(a[0]), bits(r1.centroids)), f"{what} cold"
        assert a[2] == list(r1.nsplit), f"{what} cold"
        assert np.allclose(a[1], r1.obj, rtol=2e-5, atol=0), f"{what} cold: {a[1]} against {list(r1.obj)}"
        assert np.array_equal(bits(a[3]), bits(r2.centroids)), f"{what} warm"
        assert a[5] == list(r2.nsplit), f"{what} warm"
        assert np.allclose(a[4], r2.obj, rtol=2e-5, atol=0), f"{what} warm: {a[4]} against {list(r2.obj)}"


@pytest.mark.parametrize("k,n", [(64, 4129), (1024, 8192)])
def test_training_ignores_unlisted_rows(be, oracle, settled, k, n):
    """Rows without a finite distance belong to no cluster: training on the unlisted rung from given centroids ends
    with the centroids of the same training without those rows, bit for bit -- the oracle's (it can train only the
    clean set: it indexes with the -1).  k = 64 takes the hinted path, k = 1024 the pruned one.  Before the +inf rule,
    the hinted sweep gave such a row to centroid 0 from iteration 2 on and its 2e19 went into the mean."""
    from audio_tokens_amd.ops import Kmeans
    d, niter = 64, 4
    r = md.rung(oracle, "unlisted", d, max(k, 256), n=n)
    x = r["x"]
    clean = np.setdiff1d(np.arange(n), r["overflow"])
    special = np.concatenate([r["overflow"], r["edge_sum"]])
    pool = np.setdiff1d(np.arange(n // 4 + 32, n), special)          # rows anywhere on the sphere, all distinct
    init = x[np.random.default_rng(k).choice(pool, k, replace=False)].copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ro = oracle.kmeans_train(x[clean], k, niter=niter, init_centroids=init)
        assert list(ro.nsplit) == [0] * niter
        runs = {}
        for what, rows in (("all rows", x), ("clean rows", np.ascontiguousarray(x[clean]))):
            km = Kmeans(d, k, niter=niter, backend=be)
            km.train(rows, init_centroids=init)
            runs[what] = (km.centroids.copy(), [st["nsplit"] for st in km.iteration_stats])
    assert runs["clean rows"][1] == [0] * niter
    assert np.array_equal(bits(runs["clean rows"][0]), bits(ro.centroids)), "clean rows: not the oracle's centroids"
    assert runs["all rows"][1] == [0] * niter
    diff = (bits(runs["all rows"][0]) != bits(ro.centroids)).any(axis=1)
    assert not diff.any(), f"{diff.sum()} centroids differ from the training without the unlisted rows: {np.nonzero(diff)[0][:8]}"
