"""Every exact nearest-centroid route on data far from the origin (tests/off_origin_data.py), bit for bit.

The accelerated routes promise the bits of the plain fp32 contract (ascending fmaf chains, dis = fma(-2, ip, xn + cn),
the clamp at 0, the lowest index on equal distances) for any input, but every other test feeds them data centred on
the origin, where the margins that make the shortcuts exact -- delta = (2d + 8) u (|x|^2 + max|c|^2) in the pruning
radius and in the filter's tau, the eps of the fp16 centroid-to-group bounds -- are negligible and ties are two-way.
On the ladder of off_origin_data.py (proved on the CPU by test_off_origin_ref.py) they carry the load: at offset 100
the computed distances are mostly rounding noise, whole swaths of them clamp to 0 and tie, and the lowest index has
to win across 32-centroid groups that the pruned and filtered sweeps visit in cperm order.

Shapes: n = 4129 (129 tiles of 32 + a tile of one row), k = 1000 (ng = 32, the last group padded) and k = 2080
(ng = 65: a second 64-group pass and an odd number of mask words), d = 64 and 128.  Every comparison is bit for bit
against oracle.assign, knn_ref or pq_encode_ref; the only other assertions are the float64 properties derived below.

What the tests exposed: nothing -- every route returned the oracle's bits on every rung, all three bound kernels
stayed below the truth, and the pre-pass visited at least what the lemma needs.  What they would expose: with delta
taken out of the Elkan radius (prune.hip, the fused pre-pass and the redo in filter.hip) the pruned routes return up to
161 wrong ids of 4129 on `wrong` and `flat` under the fp32 bounds, and training on `clamp` leaves the oracle's
centroids; under the fp16 bounds the same mutant passes, because those bounds are 0 at offset 100 and nothing is pruned.

MEASURED on an MI355X (the MEASURE lines; records of which regime ran, not thresholds)

Rows the filter listed for the fp32 redo, of the rows it swept (the same under all three bound kernels):
    rung     d=64 k=1000   d=64 k=2080   d=128 k=1000   d=128 k=2080
    origin   0.0249        0.0162        0.0283         0.0157
    db       0.0252        0.0165        0.0322         0.0182
    far, edge, clamp, wrong, flat: 1.0000 everywhere (tau ~ 2 delta is 20 at d = 64 and 80 at d = 128, above the gaps)

(tile, group) pairs the pre-pass kept, needed / total, fp32 sweep with true guesses; `model` is the float64 floor:
    rung     d, k        dmin_kernel 0   dmin_kernel 1   dmin_kernel 2   model
    origin   64, 1000    1854 / 4160     1854            1854            1854
    origin   64, 2080    3291 / 8450     3291            3291            3291
    origin   128, 1000   1894 / 4160     1894            1894            1894
    origin   128, 2080   3112 / 8450     3112            3112            3112
    db       64, 1000    1802 / 4160     1802            1802            1802
    db       64, 2080    2971 / 8450     2971            2971            2971
    db       128, 1000   1882 / 4160     1882            1882            1882
    db       128, 2080   3049 / 8450     3049            3049            3049
    far      64, 1000    4113 / 4160     4160            4160            1927
    far      64, 2080    8396 / 8450     8450            8450            3291
    far      128, 1000   2158 / 4160     4160            4160            1894
    far      128, 2080   4058 / 8450     8450            8450            3063
    edge, clamp, wrong, flat: needed = total under every kernel; model 0.36-0.45 of total on edge and clamp,
    0.69-0.96 on wrong, 1.0 on flat

Slack of dmin below the true minimum (k = 1000; mean true minimum 9.3 / 13.9 at the origin, 7.5 / 16.7 on far):
    origin   kernel 0: max 2.6e-4 / 3.4e-4 (d = 64 / 128)   kernel 1: 0.012 / 0.014   kernel 2: 3.5e-4 / 7.7e-4
    db       kernel 0: 2.5e-3 / 3.5e-3                      kernel 1: 2.7 / 2.5       kernel 2: 0.072 / 0.13
    far      kernel 0: 2.1e-4 / 4.1e-4      kernel 1: every bound 0 (slack = the distance)   kernel 2: max 6.2 / 7.3
    flat     kernel 0: 2.5e-6 / 3.4e-6      kernels 1 and 2: every bound 0
The fp16 bounds give up at offset 100 (their eps exceeds the squared distances) while the fp32 one keeps pruning;
at the dB-like offsets all three prune alike.

Oracle repair counts of the trainings (cold / warm): clamp d=64 [0, 20, 19, 15] / [48, 29, 32, 28], d=128
[4, 19, 17, 15] / [50, 30, 28, 27]; far and edge repair 7-14 clusters in iteration 2 cold and 117-167 in iteration 1 warm."""
import warnings

import numpy as np
import pytest
import torch

import off_origin_data as od
from knn_ref import distance_matrix, select
from pq_ref import pq_encode_ref

pytestmark = pytest.mark.gpu

N = od.N
KS = (1000, 2080)
HARD = ("clamp", "wrong", "flat")          # rungs on which the Elkan rule can skip nothing
_REF, _GMIN, _DMAT, _ARG64 = {}, {}, {}, {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ref(oracle, name, d, k):
    """(x, c, oracle ids, oracle distances) of one rung: computed once, shared, read-only."""
    key = (name, d, k)
    if key not in _REF:
        x, c = od.rung(name, d, k=k)
        ids, dis = oracle.assign(x, c)
        for a in (x, c, ids, dis):
            a.setflags(write=False)
        _REF[key] = (x, c, ids, dis)
    return _REF[key]


def _grouping(be, name, d, k, c):
    """(cperm on the host, float64 centroid-to-group minima): once per table."""
    key = (name, d, k)
    if key not in _GMIN:
        cperm = be.group_rows_kd(c)
        gmin = od.true_group_min(c, cperm)
        gmin.setflags(write=False)
        _GMIN[key] = (cperm, gmin)
    return _GMIN[key]


def _same(got, ids_o, dis_o, what, want_dist=True):
    ids, dis = got
    ids = ids.cpu().numpy()
    assert np.array_equal(ids, ids_o), f"{what}: {(ids != ids_o).sum()} of {ids.size} ids differ"
    if want_dist:
        assert np.array_equal(bits(dis.cpu().numpy()), bits(dis_o)), f"{what}: distances differ"
    else:
        assert dis is None, what


def _fp64_winner(name, d, k, x, c):
    """The float64 arg-min of every row: the guess a converged training makes, and on `wrong` and `flat` not the
    contract's winner."""
    key = (name, d, k)
    if key not in _ARG64:
        _ARG64[key] = od.facts(x, c)["arg"]
    return _ARG64[key]


def _hints(be, rng, ids_o, dis_o, k, arg64):
    truth = torch.from_numpy(ids_o).to(be.device)
    dtruth = torch.from_numpy(dis_o).to(be.device)
    n = ids_o.size
    return truth, dtruth, {
        "truth": (truth, dtruth),
        "random": (torch.from_numpy(rng.integers(0, k, n)).to(be.device), None),
        "none": (torch.full((n,), -1, dtype=torch.int64, device=be.device), None),
        "dup_high": (torch.where(truth < 20, truth + k // 2, truth), dtruth),   # the higher twin of a duplicated winner
        "mixed": (torch.where(torch.arange(n, device=be.device) % 5 == 0, (truth + 11) % k, truth), dtruth),
        "fp64": (torch.from_numpy(arg64).to(be.device), None),
    }


def _settle(be, oracle, d):
    """A filtered call on the origin rung: leaves the context in the asynchronous form for whoever comes next."""
    x, c, ids_o, dis_o = _ref(oracle, "origin", d, 1000)
    xt, ct = be._f32(x), be._f32(c)
    cperm = be.from_host(be.group_rows_kd(c))
    dmin = be.group_min_dist(ct, cperm)
    order = be.visit_order(torch.from_numpy(ids_o).to(be.device), None, 1000)
    be.filter_stats()
    for _ in range(2):
        be.assign_pruned(xt, ct, order, cperm, dmin, filter=True)
        rows, listed = be.filter_stats()
        assert listed * 16 <= rows


RUNG_CASES = [(name, d, k) for d in (64, 128) for k in KS for name in od.RUNG_NAMES]
KERNEL_CASES = [(name, d, k, dk) for (name, d, k) in RUNG_CASES for dk in (0, 1, 2)]


# ---------------------------------------------------------------------------------------------------------------------
# the dense and the hinted sweep

@pytest.mark.parametrize("name,d,k", RUNG_CASES)
def test_dense_and_hinted_sweeps(be, oracle, name, d, k):
    """assign, and assign_hinted told the truth, random ids, nothing, the higher twin of a duplicated winner and the
    float64 winner, in row order and in member-list order, with and without distances."""
    x, c, ids_o, dis_o = _ref(oracle, name, d, k)
    xt, ct = be._f32(x), be._f32(c)
    _same(be.assign(xt, ct), ids_o, dis_o, "assign")
    _same(be.assign(xt, ct, want_dist=False), ids_o, dis_o, "assign ids only", want_dist=False)
    _, _, hints = _hints(be, np.random.default_rng(d + k), ids_o, dis_o, k, _fp64_winner(name, d, k, x, c))
    for hname in ("truth", "random", "none", "dup_high", "fp64"):
        hint = hints[hname][0].contiguous()
        _, member_order = be.centroid_accum(xt, torch.clamp(hint, min=0), k, want_order=True)
        for od_name, order in (("row order", None), ("member-list order", member_order)):
            for want_dist in (True, False):
                _same(be.assign_hinted(xt, ct, hint, order, want_dist=want_dist), ids_o, dis_o,
                      f"assign_hinted hint={hname} {od_name} want_dist={want_dist}", want_dist)


@pytest.mark.parametrize("name", ["clamp", "flat"])
@pytest.mark.parametrize("d", [80, 640])
def test_generic_d_dense_sweep(be, oracle, name, d):
    """The dense sweep for any d (no MFMA form), k = 300, 1500 rows: the clamp and mass ties at 0."""
    A, s = od.RUNGS[64][name]
    x, c = od.build(9, 1500, 300, d, A, s)
    ids_o, dis_o = oracle.assign(x, c)
    assert (dis_o == 0).mean() > (0.9 if name == "flat" else 0.05)
    _same(be.assign(x, c), ids_o, dis_o, "assign")
    _same(be.assign(x, c, want_dist=False), ids_o, dis_o, "assign ids only", want_dist=False)


# ---------------------------------------------------------------------------------------------------------------------
# the pruned sweep, the fp16-split filter and its finishing paths, the unguided searches

@pytest.mark.parametrize("name,d,k,dk", KERNEL_CASES)
def test_pruned_filtered_and_unguided_routes(be, oracle, switches, name, d, k, dk):
    """assign_pruned (fp32 sweep alone / behind the filter) with true, random, missing, mixed and float64-winner
    guesses (at `flat` a random guess sits at distance 0 like the winner, which has a lower index in another group:
    only the delta in the radius keeps that group in the sweep), assign_c2f
    plain and coherent, assign_unguided, each with and without distances, under each of the three centroid-to-group
    bound kernels.  On `wrong` and `flat` also the synchronous form and the separate pre-pass, so that every
    finishing path redoes rows whose answer index order alone decides.  `flat` must list every row: tau is about
    2 delta ~ 20 (d = 64) there and no two distances are further apart than 0.1."""
    switches(dmin_kernel=dk)
    x, c, ids_o, dis_o = _ref(oracle, name, d, k)
    xt, ct = be._f32(x), be._f32(c)
    cperm = be.from_host(_grouping(be, name, d, k, c)[0])
    dmin = be.group_min_dist(ct, cperm)
    _, _, hints = _hints(be, np.random.default_rng(d + k + dk), ids_o, dis_o, k, _fp64_winner(name, d, k, x, c))
    forms = [{}]
    if name in ("wrong", "flat"):
        forms += [{"filter_sync": 1}, {"filter_fused": 0}, {"filter_sync": 1, "filter_fused": 0}]
    rows_seen = listed_seen = 0
    for form in forms:
        switches(filter_sync=0, filter_fused=1)
        switches(**form)
        for hname in ("truth", "random", "none", "mixed", "fp64"):
            hint, hd = hints[hname]
            order = be.visit_order(hint.contiguous(), hd, k)
            for flt in ((False, True) if not form else (True,)):
                for want_dist in (True, False):
                    be.filter_stats()
                    got = be.assign_pruned(xt, ct, order, cperm, dmin, want_dist=want_dist, filter=flt)
                    what = f"assign_pruned hint={hname} filter={flt} want_dist={want_dist} {form}"
                    _same(got, ids_o, dis_o, what, want_dist)
                    rows, listed = be.filter_stats()
                    assert rows == (N if flt else 0), what
                    rows_seen += rows
                    listed_seen += listed
                    if name == "flat" and flt:
                        assert listed == N, f"{what}: listed {listed} of {N}"
    switches(filter_sync=0, filter_fused=1)
    print(f"\nMEASURE {name} d={d} k={k} dmin_kernel={dk}: listed {listed_seen} of {rows_seen} filtered rows "
          f"({listed_seen / rows_seen:.4f})")
    for want_dist in (True, False):
        _same(be.assign_c2f(xt, ct, cperm, dmin, want_dist=want_dist), ids_o, dis_o, "assign_c2f", want_dist)
        _same(be.assign_c2f(xt, ct, cperm, dmin, want_dist=want_dist, coherent=True), ids_o, dis_o,
              "assign_c2f coherent", want_dist)
        _same(be.assign_unguided(xt, ct, want_dist=want_dist), ids_o, dis_o, "assign_unguided", want_dist)
        _same(be.assign_unguided(xt, ct, want_dist=want_dist, cperm=cperm), ids_o, dis_o, "assign_unguided kd", want_dist)
    _settle(be, oracle, d)


@pytest.mark.parametrize("name,d,k,dk", KERNEL_CASES)
def test_dmin_is_a_lower_bound_everywhere(be, oracle, switches, name, d, k, dk):
    """dmin[p][g] <= the true min over the members of group g of |c_p - c_m|, for every p and every g, compared in
    float64.  The reference is the float64 sum of d squared differences, within (d + 2) 2^-53 < 1e-13 relative of the
    truth: hence the factor 1 + 1e-12 and nothing else.  A group of padding only reads +inf.  The bound is held to be
    useful (within 0.02) only at the origin with the fp32 kernel; elsewhere its slack is printed: the fp16 kernels
    give up at offset 100 (their eps is of the order of the distances), which is safe."""
    switches(dmin_kernel=dk)
    x, c, _, _ = _ref(oracle, name, d, k)
    cperm, gmin = _grouping(be, name, d, k, c)
    got = be.group_min_dist(be._f32(c), be.from_host(cperm)).cpu().numpy().astype(np.float64)
    assert got.shape == gmin.shape and not np.isnan(got).any()
    assert np.isfinite(gmin).all()
    over = got > gmin * (1.0 + 1e-12)
    assert not over.any(), f"{over.sum()} bounds above the truth, worst by {(got - gmin)[over].max():.3e}"
    slack = gmin - got
    print(f"\nMEASURE {name} d={d} k={k} dmin_kernel={dk}: slack of dmin max {slack.max():.4g}, mean {slack.mean():.4g}; "
          f"true minima mean {gmin.mean():.4g}; bounds at 0: {(got == 0).mean():.3f}")
    if name == "origin" and dk == 0:
        assert slack.max() <= 0.02
    if k == 1000:
        # the same table with a group of padding only behind it: +inf there, the other columns unchanged
        padded = np.concatenate([cperm, np.full(32, -1, np.int32)])
        got2 = be.group_min_dist(be._f32(c), be.from_host(padded)).cpu().numpy()
        assert got2.shape == (k, gmin.shape[1] + 1)
        assert np.isposinf(got2[:, -1]).all()
        assert np.array_equal(got2[:, :-1].astype(np.float64), got)


def _needed_model(x, c, k, order, hint_sorted, gmin):
    """The (32-position tile, group) pairs no correct pruning can skip: some row r of the tile, guessed p, has
    true_min_dist(c_p, group) <= 2 sqrt(T(x_r, c_p)) (1 - 1e-9) with T the true squared distance -- no delta, no
    inflation; a row without a guess needs every group."""
    o = order.cpu().numpy().view(np.uint32).astype(np.int64)
    p = hint_sorted.cpu().numpy().view(np.uint32).astype(np.int64)
    has = p < k
    pc = np.where(has, p, 0)
    T = od.true_rowwise_sqdist(x[o], c[pc])
    thr = 2.0 * np.sqrt(T) * (1.0 - 1e-9)
    need = gmin[pc] <= thr[:, None]
    need[~has] = True
    ntile = (o.size + 31) // 32
    full = np.zeros((ntile * 32, gmin.shape[1]), bool)
    full[:o.size] = need
    return int(full.reshape(ntile, 32, -1).any(axis=1).sum())


@pytest.mark.parametrize("name,d,k,dk", KERNEL_CASES)
def test_pruning_never_skips_what_the_lemma_cannot_justify(be, oracle, switches, name, d, k, dk):
    """One assign_pruned call (fp32 sweep, true guesses with their distances) and the pre-pass counters: every
    (tile, group) pair is accounted for, and at least the pairs the float64 model needs are visited -- any correct
    implementation has a larger radius and a smaller dmin than the model.  `far` really prunes with the fp32 bounds;
    `clamp`, `wrong` and `flat` cannot prune at all (the Elkan share in exact arithmetic is 0 there)."""
    switches(dmin_kernel=dk)
    x, c, ids_o, dis_o = _ref(oracle, name, d, k)
    xt, ct = be._f32(x), be._f32(c)
    cperm_h, gmin = _grouping(be, name, d, k, c)
    cperm = be.from_host(cperm_h)
    ng = cperm_h.size // 32
    dmin = be.group_min_dist(ct, cperm)
    order = be.visit_order(torch.from_numpy(ids_o).to(be.device), torch.from_numpy(dis_o).to(be.device), k)
    be.prune_stats(reset=True)
    _same(be.assign_pruned(xt, ct, order, cperm, dmin, filter=False), ids_o, dis_o, "assign_pruned")
    needed, total = be.prune_stats()
    model = _needed_model(x, c, k, order[0], order[1], gmin)
    print(f"\nMEASURE {name} d={d} k={k} dmin_kernel={dk}: needed {needed} of {total} ({needed / total:.4f}), "
          f"model {model} ({model / total:.4f})")
    assert total == ng * ((N + 31) // 32)
    assert needed >= model
    if name == "far" and dk == 0:
        assert needed < total
    if name in HARD:
        assert needed == total


# ---------------------------------------------------------------------------------------------------------------------
# k nearest centroids and the PQ encoder on the same data

def _dmat(oracle, name, d):
    key = (name, d)
    if key not in _DMAT:
        x, c, _, _ = _ref(oracle, name, d, 1000)
        D, ok = distance_matrix(oracle, x, c)
        D.setflags(write=False)
        ok.setflags(write=False)
        _DMAT[key] = (D, ok)
    return _DMAT[key]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", ["edge", "clamp", "wrong", "flat"])
def test_knn_lists_under_mass_ties(be, oracle, name, d):
    """be.knn with k = 8 and 32 (the fused lists) and 40 (the general path) against knn_ref at k_c = 1000.  At `flat`
    the list of most rows is simply the lowest ids at distance 0: the per-lane strict-< insert and the half-wave
    merge have to keep index order among hundreds of equal keys."""
    x, c, ids_o, dis_o = _ref(oracle, name, d, 1000)
    D, ok = _dmat(oracle, name, d)
    xt, ct = be._f32(x), be._f32(c)
    for kk in (8, 32, 40):
        Dr, Ir = select(D, ok, kk)
        assert np.array_equal(Ir[:, 0], ids_o)
        if name == "flat":
            assert (Dr[:, :32] == 0).all(axis=1).mean() > 0.5
        I, Dg = be.knn(xt, ct, kk)
        I, Dg = I.cpu().numpy(), Dg.cpu().numpy()
        assert np.array_equal(I, Ir), f"k={kk}: {(I != Ir).any(axis=1).sum()} of {N} lists differ"
        assert np.array_equal(bits(Dg), bits(Dr)), f"k={kk}"
        I2, none = be.knn(xt, ct, kk, want_dist=False)
        assert none is None and np.array_equal(I2.cpu().numpy(), Ir), f"k={kk} ids only"


@pytest.mark.parametrize("M", [8, 16])
@pytest.mark.parametrize("name", ["edge", "clamp", "wrong", "flat"])
def test_pq_encoder_off_origin(be, oracle, name, M):
    """be.pq_encode at d = 64 with M = 8 (dsub 8) and M = 16 (dsub 4), codebook m = the first 256 centroids' slice m,
    against pq_encode_ref; and the first 19 rows alone, which take the direct form (sum of squared differences) and
    do not cancel."""
    x, c, _, _ = _ref(oracle, name, 64, 1000)
    dsub = 64 // M
    cb = np.ascontiguousarray(np.stack([c[:256, m * dsub:(m + 1) * dsub] for m in range(M)]))
    for rows in (x, x[:19]):
        codes_r, dist_r, bad_r = pq_encode_ref(oracle, rows, cb)
        assert not bad_r
        codes, dist, bad = be.pq_encode(np.ascontiguousarray(rows), cb, want_dist=True)
        codes = codes.cpu().numpy()
        assert np.array_equal(codes, codes_r), f"n={rows.shape[0]}: {(codes != codes_r).sum()} codes differ"
        assert np.array_equal(bits(dist.cpu().numpy()), bits(dist_r)), f"n={rows.shape[0]}"
        assert int(bad.cpu()[0]) == 0
        codes2, none, _ = be.pq_encode(np.ascontiguousarray(rows), cb)
        assert none is None and np.array_equal(codes2.cpu().numpy(), codes_r)


# ---------------------------------------------------------------------------------------------------------------------
# training

@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", ["far", "edge", "clamp"])
def test_training_off_origin(be, oracle, switches, name, d):
    """Kmeans(d, 1024, niter=4) on 8192 rows, then a warm start on another 8192 (both prune: n >= 4096, k >= 1024),
    pruned and dense, under the fp32 and the default fp16 centroid-to-group bounds: centroids and repair counts the
    oracle's bit for bit, objectives within the suite's rtol 2e-5 of it and equal between pruned and dense runs.
    On `clamp` the oracle repairs clusters in every iteration, so split_clusters runs on the device too."""
    from audio_tokens_amd.ops import Kmeans
    k, n1, niter = 1024, 8192, 4
    A, s = od.RUNGS[d][name]
    x, _ = od.build(9, 2 * n1, k, d, A, s)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r1 = oracle.kmeans_train(x[:n1], k, niter=niter)
        r2 = oracle.kmeans_train(x[n1:], k, niter=niter, init_centroids=r1.centroids)
        print(f"\nMEASURE training {name} d={d}: oracle nsplit cold {list(r1.nsplit)} warm {list(r2.nsplit)}")
        if name == "clamp":
            assert sum(r1.nsplit) > 0 and sum(r2.nsplit) > 0
        got = {}
        for dk in (0, 1):
            switches(dmin_kernel=dk)
            for prune in (True, False):
                km = Kmeans(d, k, niter=niter, backend=be)
                km.prune = prune
                km.train(x[:n1])
                cold = (km.centroids.copy(), list(km.obj), [st["nsplit"] for st in km.iteration_stats])
                km.train(x[n1:], init_centroids=km.centroids)
                got[dk, prune] = cold + (km.centroids.copy(), list(km.obj), [st["nsplit"] for st in km.iteration_stats])
    for (dk, prune), a in got.items():
        what = f"dmin_kernel={dk} prune={prune}"
        assert np.array_equal(bits(a[0]), bits(r1.centroids)), f"{what} cold"
        assert a[2] == list(r1.nsplit), f"{what} cold"
        assert np.allclose(a[1], r1.obj, rtol=2e-5, atol=0), f"{what} cold"
        assert np.array_equal(bits(a[3]), bits(r2.centroids)), f"{what} warm"
        assert a[5] == list(r2.nsplit), f"{what} warm"
        assert np.allclose(a[4], r2.obj, rtol=2e-5, atol=0), f"{what} warm"
        b = got[dk, False]
        assert a[1] == b[1] and a[4] == b[4], f"{what}: objectives differ from the dense run's"
    _settle(be, oracle, d)
