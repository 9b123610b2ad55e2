"""The layer beneath the exact nearest-centroid search, looked at directly: the group means, the centroid-to-group
bounds, the per-tile group masks of the pre-pass (separate and fused into the filter sweep) and the two guess
generators (guess mode of at_assign_pruned_f32, at_assign_coarse_f32), each against the float64 models of
tests/guess_ref.py.  The exact routes return the dense sweep's bits whatever this layer does, so every other test stays
green when a generator searches the wrong groups or a mask carries a wrong bit; only the speed decays.

tests/test_guess_ref.py proves on the CPU that the inputs used here leave something to prune and something to keep
(the caps and the values found: DESIGN.md section 5.0d, with the MEASURE lines of one run of this file).

Shapes: d in {64, 128}; n in {33, 127, 128, 129, 2033} (the coarse kernel takes 128 rows per workgroup at d = 64 and 64
at d = 128, the pre-pass 64 positions per wave: two tiles); k / ng = 33 / 2 (a second group of one live slot),
1285 / 41 (two mask words), 2085 / 66 (a second 64-group pass with a 2-group tail), 16384 / 512 (the size limit: all 8
passes, 16 mask words).  Groupings: be.group_rows_kd, and a hand-made one whose groups carry padding slots in the
middle, followed by a group of padding only.  Both image builders (prep_centroids_f16_kernel in filter.hip,
prep_centroids_perm_kernel in assign.hip) test every slot for row >= 0 on its own and give a padding slot |c|^2 = +inf,
wherever it sits, so the hand-made grouping goes through the sweeps as well: the separate and the fused pre-pass,
guess mode and the coarse pass each run it at k = 1285 (44 groups), d = 64 and 128.

What was corrected in the models while writing the tests: the walk of the coarse pass over the group means keeps the
hi*hi product only (assign_f16filter_kernel, `means_walk`), so the mean a row names is within 2 (filter_eps +
filter_rho) of the nearest, not within 2 filter_eps; coarse_sets is fed that eps, and the tables of the coarse tests
are the ones on which the caps hold with it (guess_ref.COARSE_TABLES)."""
import numpy as np
import pytest
import torch

import guess_ref as gr
import off_origin_data as od
from audio_tokens_amd import _lib
from audio_tokens_amd.backend import _ptr

pytestmark = pytest.mark.gpu

_KD, _ORACLE, _GMIN = {}, {}, {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(be, a):
    return be.from_host(np.array(a))


def _kd(be, key, c):
    """The kd grouping of a table on the host: once per table."""
    if key not in _KD:
        _KD[key] = be.group_rows_kd(c)
    return _KD[key]


def _oracle(oracle, key, x, c):
    """(ids, distances) of the oracle for the 2033 rows of a table: once, shared, read-only (a prefix of the rows has a
    prefix of the answers)."""
    if key not in _ORACLE:
        ids, dis = oracle.assign(x, c)
        ids.setflags(write=False)
        dis.setflags(write=False)
        _ORACLE[key] = (ids, dis)
    return _ORACLE[key]


def _order_tensors(be, order, hs):
    return _dev(be, order.astype(np.int32)), _dev(be, hs.astype(np.int32))


def _settle(be, oracle, d):
    """Two filtered calls on well-behaved rows.  A call that lists more than n/16 rows (three rows of 33 do) makes the
    context finish its next exact calls synchronously, and a synchronous call with a long list runs a SECOND pre-pass
    over the listed rows, which adds to the counters and overwrites bd and the masks.  No switch forces the
    asynchronous form (filter_sync = 1 forces the other one), so the test puts the context back into it the way the
    library itself does: by a call whose list is short."""
    key = ("origin", d, 1285, 5, gr.NSUPER)
    x, c = gr.table(*key)
    ids_o, _ = _oracle(oracle, key, x, c)
    xt, ct = _dev(be, x), _dev(be, c)
    cperm = _dev(be, _kd(be, key, c))
    order = be.visit_order(_dev(be, ids_o), None, 1285)
    dmin = be.group_min_dist(ct, cperm)
    be.filter_stats()
    for _ in range(2):
        be.assign_pruned(xt, ct, order, cperm, dmin, filter=True)
        rows, listed = be.filter_stats()
        assert listed * 16 <= rows


# ---------------------------------------------------------------------------------------------------------------------
# (a) group means

@pytest.mark.parametrize("d", [64, 128, 8, 300])
def test_group_means_bit_for_bit(be, d):
    """be.group_means against group_means_model, bit for bit: k = 1285 (the last group has 5 live slots), values of
    mixed magnitude so that the order of the fp32 sum shows; the kd grouping, the hand-made grouping with padding in
    the middle of every group and a group of padding only (means 0), and a shuffled grouping.  d = 300 exceeds one
    pass of the kernel's 256 threads."""
    rng = np.random.default_rng(d)
    k = 1285
    c = (rng.standard_normal((k, d)) * rng.choice([1e-3, 1.0, 300.0], (k, d))).astype(np.float32)
    kd = be.group_rows_kd(c)
    shuffled = np.full(41 * 32, -1, np.int32)
    shuffled[rng.permutation(41 * 32)[:k]] = rng.permutation(k)
    for what, cperm in (("kd", kd), ("padded", gr.kd_padded_cperm(kd)), ("shuffled", shuffled)):
        want = gr.group_means_model(c, cperm)
        got = be.group_means(_dev(be, c), _dev(be, cperm)).cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), f"{what}: {(bits(got) != bits(want)).sum()} of {got.size} values differ"
        if what == "padded":
            assert np.array_equal(bits(got[-1]), np.zeros(d, np.uint32))
    # dividing by 32 instead of the live count would go unnoticed on full groups only
    assert (np.asarray(kd).reshape(-1, 32)[-1] >= 0).sum() == k - 40 * 32


# ---------------------------------------------------------------------------------------------------------------------
# (b) centroid-to-group bounds

@pytest.mark.parametrize("k", [33, 1285, 2085, 16384])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", gr.MASK_RUNGS)
def test_group_min_dist_both_forms(be, switches, name, d, k):
    """dmin[p][g] of the fp32 kernel (dmin_kernel = 0) and of the default fp16 hi*hi kernel against the float64 truth
    (od.true_group_min), every group, every p (at k = 16384 every 23rd p and the first and last 64: the truth of all
    of them is a 2 GiB matrix), on the kd grouping and on the hand-made one with interior padding:
        dmin <= truth (x (1 + 1e-12): the truth is a float64 sum of d squared differences);
        +inf exactly for the group of padding only; 0 exactly for the centroid's own group;
        fp32 form: dmin >= truth (1 - 1e-4): the kernel shaves 2e-5 off the root of a sum within (d + 3) 2^-24;
        fp16 form: the kernel returns (1 - 1e-6) sqrt(max(P + |c_p|^2 - B, 0)) with P the smallest hi*hi value of
        the group and B = eps_a (1.001 |c_p|^2 + max|c|^2) + eps_b, the bound on |P + |c_p|^2 - T| that it subtracts
        (guess_ref.dmin_f16_bound, constants of at_group_min_dist_f16).  So P + |c_p|^2 >= T - B and
            dmin^2 >= (1 - 4e-6) (T - 2.01 B):
        2 B from the error and the subtraction, 0.01 B >= 1e-5 H for the three fp32 roundings of forming the value
        (6 x 2^-24 H with H = |c_p|^2 + max|c|^2 >= the magnitudes involved), 4e-6 for (1 - 1e-6)^2 and the root."""
    key = (name, d, k, 5, gr.NSUPER)
    _, c = gr.table(*key)
    ct = _dev(be, c)
    kd = _kd(be, key, c)
    rows = np.arange(k) if k <= 4096 else np.unique(np.concatenate([np.arange(64), np.arange(0, k, 23), np.arange(k - 64, k)]))
    cn = gr.sq_norms(c)
    for what, cperm in (("kd", kd), ("padded", gr.kd_padded_cperm(kd))):
        if what == "padded" and k > 4096:
            continue
        gkey = key + (what,)
        if gkey not in _GMIN:
            _GMIN[gkey] = od.true_group_min(c, cperm) if k <= 4096 else gr.group_min_rows(c, cperm, rows)
        true = _GMIN[gkey]
        own = gr.group_of(cperm, k)
        for dk in (0, 1):
            switches(dmin_kernel=dk)
            full = be.group_min_dist(ct, _dev(be, cperm)).cpu().numpy().astype(np.float64)
            got = full[rows]
            assert got.shape == true.shape and not np.isnan(full).any()
            over = got > true * (1.0 + 1e-12)
            assert not over.any(), f"{what} dk={dk}: {over.sum()} bounds above the truth"
            assert (full[np.arange(k), own] == 0.0).all(), f"{what} dk={dk}: own group not at 0"
            if what == "padded":
                assert np.isposinf(full[:, -1]).all() and np.isposinf(true[:, -1]).all()
                assert np.isfinite(full[:, :-1]).all()
            fin = np.isfinite(true)
            if dk == 0:
                ratio = np.min(got[fin & (true > 0)] / true[fin & (true > 0)])
                print(f"\nMEASURE {name} d={d} k={k} {what} fp32 form: smallest dmin / truth {ratio:.7f}")
                assert (got[fin] >= true[fin] * (1.0 - 1e-4)).all()
            else:
                B = gr.dmin_f16_bound(d, cn[rows], cn.max())[:, None]
                floor = (1.0 - 4e-6) * (true ** 2 - 2.01 * B)
                used = np.max((true[fin] ** 2 - got[fin] ** 2) / (2.0 * np.broadcast_to(B, true.shape)[fin]))
                print(f"\nMEASURE {name} d={d} k={k} {what} fp16 form: largest (truth^2 - dmin^2) / 2B {used:.4f}; "
                      f"bounds at 0: {(got == 0).mean():.3f}")
                assert (got[fin] ** 2 >= floor[fin]).all()


# ---------------------------------------------------------------------------------------------------------------------
# (c), (d) the pre-pass: bd and the masks, separate and fused

def _prepass_case(be, oracle, switches, name, d, n, k, none_tail, padded, forms):
    """Runs the separate pre-pass (fp32 sweep behind it) under each dmin form, checks bd and every mask bit, and
    returns per form (popcount, must, may, cperm tensor, dmin tensor, order tensors)."""
    key = (name, d, k, 5, gr.NSUPER)
    m = gr.mask_inputs(name, d, n, k, none_tail)
    x, c, order, hs, has = m["x"], m["c"], m["order"], m["hs"], m["has"]
    ids_o, dis_o = _oracle(oracle, key, *gr.table(*key))
    ids_o, dis_o = ids_o[:n], dis_o[:n]
    kd = _kd(be, key, c)
    cperm_h = gr.kd_padded_cperm(kd) if padded else kd
    ng = cperm_h.size // 32
    ntile = (n + 31) // 32
    xt, ct, cperm = _dev(be, x), _dev(be, c), _dev(be, cperm_h)
    ot = _order_tensors(be, order, hs)
    T_guess = m["T"][order, np.where(has, hs, 0)]
    delta = od.delta_bound(x[order], c)
    xn, cnmax = gr.sq_norms(x[order]), gr.sq_norms(c).max()
    out = {}
    for dk in forms:
        switches(dmin_kernel=dk, filter_fused=0)
        dmin = be.group_min_dist(ct, cperm)
        be.prune_stats(reset=True)
        ids, dis = be.assign_pruned(xt, ct, ot, cperm, dmin, filter=False)
        bd, mask = be.prune_peek(n, ng)
        needed, total = be.prune_stats(reset=True)
        what = f"{name} d={d} n={n} k={k} none_tail={none_tail} padded={padded} dmin_kernel={dk}"
        assert np.array_equal(ids.cpu().numpy(), ids_o) and np.array_equal(bits(dis.cpu().numpy()), bits(dis_o)), what
        bd = bd.cpu().numpy()
        assert np.isposinf(bd[~has]).all(), what
        assert (np.abs(bd[has].astype(np.float64) - T_guess[has]) <= delta[has]).all(), what
        right = has & (hs == ids_o[order])
        assert right.sum() > n // 2
        assert np.array_equal(bits(bd[right]), bits(dis_o[order][right])), what
        every = gr.bits_to_bool(mask.cpu().numpy(), ng)
        assert every.shape == (ntile, (ng + 31) // 32 * 32)
        assert not every[:, ng:].any(), f"{what}: bits at or beyond ng set"
        got = every[:, :ng]
        must, may = gr.mask_bracket(bd, hs, has, dmin.cpu().numpy(), xn, cnmax, d)
        print(f"\nMEASURE {what}: needed {needed} of {total} ({needed / total:.4f}); must {must.sum()}, may {may.sum()}")
        assert not (must & ~got).any(), f"{what}: {(must & ~got).sum()} needed bits missing"
        assert not (got & ~may).any(), f"{what}: {(got & ~may).sum()} bits set that no row needs"
        assert needed == got.sum() and total == ng * ntile, what
        out[dk] = (int(got.sum()), int(must.sum()), int(may.sum()), cperm, dmin, ot)
    return xt, ct, ids_o, dis_o, ng, ntile, out


@pytest.mark.parametrize("name,d,n,k,none_tail", gr.MASK_CASES)
def test_prepass_bd_and_masks_bit_by_bit(be, oracle, switches, name, d, n, k, none_tail):
    """at_prune_mask_f32 + the fp32 sweep, then at_prune_peek.  Guesses: the float64 winner with its distance, 10 % of
    the rows their second-nearest centroid (tiles hold several runs, with radii that reach other groups), every 37th
    row none -- or the last 17 / 97 rows none, which start at a tile boundary inside a wave / in the middle of a
    wave's first tile.  bd: within delta_bound of the truth, the oracle's bits where the guess is the oracle's winner,
    +inf without a guess.  Masks: every `must` bit set, no bit outside `may`, none at or beyond ng; mask_bracket is fed
    the device's own dmin and bd, so this isolates the mask logic (run leaders, the two tiles of a wave, the tail of
    the last 64-group word, tau) from the two inputs checked on their own.  Counters: needed = popcount, total =
    ng x tiles.  Under the fp32 bounds, and under the default fp16 ones (which are 0 at offset 100: on `far` they
    keep every pair)."""
    _prepass_case(be, oracle, switches, name, d, n, k, none_tail, False, (0, 1))


@pytest.mark.parametrize("d", [64, 128])
def test_prepass_masks_with_interior_padding(be, oracle, switches, d):
    """The same on the hand-made grouping (44 groups of 30 + padding in the middle, the last of padding only: its dmin
    is +inf, so its bit is set only in tiles that hold a row without a guess)."""
    _prepass_case(be, oracle, switches, "origin", d, 2033, 1285, None, True, (0, 1))


FUSED_CASES = ([(r, d, 2033, 33) for r in gr.MASK_RUNGS for d in (64, 128)]
               + [(r, d, n, 1285) for r in gr.MASK_RUNGS for d in (64, 128) for n in gr.NS]
               + [(r, d, 2033, 2085) for r in gr.MASK_RUNGS for d in (64, 128)]
               + [("far", d, 2033, 16384) for d in (64, 128)])
FUSED_CASES = [case + (False,) for case in FUSED_CASES] + [("origin", d, 2033, 1285, True) for d in (64, 128)]


@pytest.mark.parametrize("name,d,n,k,padded", FUSED_CASES)
def test_fused_prepass_counts(be, oracle, switches, name, d, n, k, padded):
    """The pre-pass fused into the filter sweep (the default route) keeps no masks: its counters are held against the
    separate pre-pass of the same call.  The fused code evaluates the same three ascending fmaf chains (the chain
    state hops between the two lanes that hold a row), the same delta and tau expressions and the same test
    dmin[p][g] <= max tau of the run, so its bd and its masks are the separate kernel's, bit for bit: needed is
    asserted EQUAL to the separate pre-pass's popcount (hence inside [popcount(must), popcount(may)]), total =
    ng x tiles, under filter_nb = 0 (the default choice), 1, 2 and 4 tiles per wave.  The last two cases run on the
    hand-made grouping with interior padding and a group of padding only."""
    forms = (0,) if name == "far" else (1,)          # (the fp16 bounds are 0 on `far`: nothing to count)
    xt, ct, ids_o, dis_o, ng, ntile, out = _prepass_case(be, oracle, switches, name, d, n, k, None, padded, forms)
    pop, must, may, cperm, dmin, ot = out[forms[0]]
    # the separate pre-pass in front of the filter sweep: same masks
    _settle(be, oracle, d)
    switches(filter_fused=0, filter_stats=1)
    be.prune_stats(reset=True)
    ids, dis = be.assign_pruned(xt, ct, ot, cperm, dmin, filter=True)
    assert np.array_equal(ids.cpu().numpy(), ids_o) and np.array_equal(bits(dis.cpu().numpy()), bits(dis_o))
    _, mask = be.prune_peek(n, ng)
    assert int(gr.bits_to_bool(mask.cpu().numpy(), ng).sum()) == pop
    for nb in (0, 1, 2, 4):
        switches(filter_fused=1, filter_stats=0, filter_nb=0)
        _settle(be, oracle, d)
        switches(filter_fused=1, filter_stats=1, filter_nb=nb)
        be.prune_stats(reset=True)
        ids, dis = be.assign_pruned(xt, ct, ot, cperm, dmin, filter=True)
        needed, total = be.prune_stats(reset=True)
        what = f"{name} d={d} n={n} k={k} padded={padded} filter_nb={nb}"
        assert np.array_equal(ids.cpu().numpy(), ids_o) and np.array_equal(bits(dis.cpu().numpy()), bits(dis_o)), what
        print(f"\nMEASURE {what}: fused needed {needed} of {total}; separate {pop}; must {must}, may {may}")
        assert total == ng * ntile, what
        assert must <= needed <= may, what
        assert needed == pop, what
    switches(filter_fused=1, filter_stats=0, filter_nb=0)
    _settle(be, oracle, d)


# ---------------------------------------------------------------------------------------------------------------------
# (e) guess mode of at_assign_pruned_f32

GUESS_CASES = ([(r, d, 2033, 1285, False) for r in gr.MASK_RUNGS for d in (64, 128)]
               + [("origin", d, n, k, False) for d in (64, 128) for (n, k) in ((33, 33), (129, 1285), (2033, 2085), (2033, 16384))]
               + [("origin", d, 2033, 1285, True) for d in (64, 128)])


@pytest.mark.parametrize("name,d,n,k,padded", GUESS_CASES)
def test_guess_mode_searches_its_tile_candidates(be, name, d, n, k, padded):
    """be.assign_pruned(..., mode=1): the rows name random groups and are visited in be.visit_order of those names;
    with gnbr = None and with be.group_neighbours tables of 1, 4 and 8 neighbours; through the fp32 sweep (tol =
    delta_bound) and through the fp16-split sweep (tol = filter_eps).  Per 32-position tile the candidates are
    tile_candidates: every id is a live member of a candidate group, true_dist(id) <= the smallest true distance among
    the candidates + 2 tol, |dist - true_dist(id)| <= tol, and -1 (with dist = +inf) exactly where the tile's
    candidates have no live member (the hand-made grouping's group of padding only, named without a table)."""
    key = (name, d, k, 5, gr.NSUPER)
    x, c = gr.table(*key)
    x = x[:n]
    T = gr.truth(*key)[:n]
    kd = _kd(be, key, c)
    cperm_h = gr.kd_padded_cperm(kd) if padded else kd
    ng = cperm_h.size // 32
    own = gr.group_of(cperm_h, k)
    xt, ct, cperm = _dev(be, x), _dev(be, c), _dev(be, cperm_h)
    means = be.group_means(ct, cperm)
    rng = np.random.default_rng(n + k + d)
    g = rng.integers(0, ng, n)
    order, gs_t = be.visit_order(_dev(be, g), None, ng)
    o = order.cpu().numpy().view(np.uint32).astype(np.int64)
    gs = gs_t.cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(np.sort(o), np.arange(n)) and np.array_equal(gs, g[o]) and (np.diff(gs) >= 0).all()
    To = T[o]
    tile = np.arange(n) // 32
    tols = {False: od.delta_bound(x[o], c), True: gr.filter_eps(d, gr.sq_norms(x[o]) + gr.sq_norms(c).max())}
    best = T.argmin(axis=1)[o]
    for nnb in (None, 1, 4, 8):
        gnbr = None if nnb is None else be.group_neighbours(means, nnb)
        cand = gr.tile_candidates(gs, None if gnbr is None else gnbr.cpu().numpy(), ng)
        assert cand.any(axis=1).all()
        if nnb is not None:
            assert (cand.sum(axis=1) >= min(nnb, ng)).all()
        ok = cand[:, own][tile]                                   # [n, k]: centroid j is a candidate of position i
        floor = np.where(ok, To, np.inf).min(axis=1)
        for flt in (False, True):
            ids, dist = be.assign_pruned(xt, ct, (order, gs_t), cperm, gnbr, mode=1, filter=flt)
            ids, dist = ids.cpu().numpy()[o], dist.cpu().numpy()[o].astype(np.float64)
            what = f"{name} d={d} n={n} k={k} padded={padded} nnb={nnb} filter={flt}"
            none = np.isinf(floor)
            assert padded or not none.any()
            assert ((ids == -1) == none).all(), f"{what}: -1 where candidates exist, or an id where none does"
            assert np.isposinf(dist[none]).all(), what
            live = ~none
            assert ((ids[live] >= 0) & (ids[live] < k)).all(), what
            assert ok[live, ids[live]].all(), f"{what}: {(~ok[live, ids[live]]).sum()} ids outside the tile's candidates"
            t_id = To[live, ids[live]]
            tol = tols[flt][live]
            assert (t_id <= floor[live] + 2.0 * tol).all(), what
            assert (np.abs(dist[live] - t_id) <= tol).all(), what
            print(f"\nMEASURE {what}: candidates {cand.mean():.3f} of the pairs; guess is the true nearest for "
                  f"{(ids == best).mean():.4f} of the rows, the best candidate for {(t_id == floor[live]).mean():.4f}")


@pytest.mark.parametrize("k", [1285, 16384])
def test_nearest_mean_through_the_all_ones_table(be, k):
    """be._nearest_mean at d = 64: guess mode over an image of the group MEANS with a table of all ones (every bit of
    every word, also those beyond the number of groups): the group it names is within 2 filter_eps of the true nearest
    mean and is a group that exists."""
    d, key = 64, ("origin", 64, k, 5, gr.NSUPER)
    x, c = gr.table(*key)
    cperm = _dev(be, _kd(be, key, c))
    assert be.switches["filter"]
    means = be.group_means(_dev(be, c), cperm)
    got = be._nearest_mean(_dev(be, x), means).cpu().numpy()
    mh = means.cpu().numpy()
    T = od.true_sqdist(x, mh)
    assert ((got >= 0) & (got < mh.shape[0])).all()
    eps = gr.filter_eps(d, gr.sq_norms(x) + gr.sq_norms(mh).max())
    assert (T[np.arange(x.shape[0]), got] <= T.min(axis=1) + 2.0 * eps).all()
    print(f"\nMEASURE nearest mean k={k}: the true nearest for {(got == T.argmin(axis=1)).mean():.4f} of the rows")


# ---------------------------------------------------------------------------------------------------------------------
# (f) at_assign_coarse_f32

def _coarse_guarded(be, xt, ct, cperm, means, gnbr, guard=64):
    """at_assign_coarse_f32 into buffers with `guard` sentinel entries behind the n it may write."""
    n, d = xt.shape
    ids = torch.full((n + guard,), -7, dtype=torch.int64, device=be.device)
    dist = torch.full((n + guard,), -7.0, dtype=torch.float32, device=be.device)
    with torch.cuda.device(be.device):
        _lib.check(be.lib.at_assign_coarse_f32(be.ctx.handle, _ptr(xt), n, d, _ptr(ct), ct.shape[0], _ptr(cperm),
                                                cperm.numel() // 32, _ptr(means), _ptr(gnbr), _ptr(ids), _ptr(dist),
                                                be._stream()))
    ids, dist = ids.cpu().numpy(), dist.cpu().numpy()
    assert (ids[n:] == -7).all() and (dist[n:] == -7.0).all(), "the last tile's missing rows wrote something"
    return ids[:n], dist[:n].astype(np.float64)


def _coarse_case(be, key, x, c, T, cperm_h, what0):
    """One table, one grouping, neighbour tables of 1, 4 and 8 groups: the assertions of the coarse pass.  A tile whose
    upper set has no live member must answer -1 and +inf; one whose lower set has a live member must answer an id."""
    n, d = x.shape
    k = c.shape[0]
    ng = cperm_h.size // 32
    own = gr.group_of(cperm_h, k)
    live = np.bincount(own, minlength=ng) > 0
    xt, ct, cperm = _dev(be, x), _dev(be, c), _dev(be, cperm_h)
    means = be.group_means(ct, cperm)
    mh = means.cpu().numpy()
    eps, eps_m = gr.coarse_eps(d, x, c)
    tile = np.arange(n) // 32
    best = T.argmin(axis=1)
    near = od.true_sqdist(x, mh).argmin(axis=1)
    seen_dead = 0
    for nnb in (1, 4, 8):
        gnbr = be.group_neighbours(means, nnb)
        gh = gnbr.cpu().numpy()
        L, U, adm = gr.coarse_sets(x, mh, gh, eps_m)
        assert L.any(axis=1).all()
        ids, dist = _coarse_guarded(be, xt, ct, cperm, means, gnbr)
        what = f"{what0} nnb={nnb}"
        dead = ~(U & live).any(axis=1)[tile]                      # nothing live that the tile may search
        sure = (L & live).any(axis=1)[tile]                       # something live that it must search
        assert (sure | dead).all(), what
        seen_dead += int(dead.sum())
        assert (ids[dead] == -1).all() and np.isposinf(dist[dead]).all(), f"{what}: an id out of groups of padding only"
        ids_s, t_s = ids[sure], T[sure]
        assert ((ids_s >= 0) & (ids_s < k)).all(), what
        assert U[tile[sure], own[ids_s]].all(), f"{what}: {(~U[tile[sure], own[ids_s]]).sum()} ids outside the upper set"
        t_id = t_s[np.arange(ids_s.size), ids_s]
        floor = np.where(L[:, own][tile[sure]], t_s, np.inf).min(axis=1)
        assert np.isfinite(floor).all()
        assert (t_id <= floor + 2.0 * eps[sure]).all(), what
        assert (np.abs(dist[sure] - t_id) <= eps[sure]).all(), what
        # the contract in float64: nearest mean, the tile's union of its table rows, the best centroid in there
        model = np.where(gr.tile_candidates(near, gh, ng)[:, own][tile], T, np.inf).argmin(axis=1)
        print(f"\nMEASURE {what}: guess is the true nearest for {(ids == best).mean():.4f} of the rows, float64 model "
              f"{(model == best).mean():.4f}; ambiguous means {(adm.sum(axis=1) > 1).sum()} rows; L {L.mean():.3f} U {U.mean():.3f}")
    return seen_dead


@pytest.mark.parametrize("d,n,k", gr.COARSE_CASES)
def test_coarse_pass_searches_what_its_means_name(be, d, n, k):
    """at_assign_coarse_f32 on rows in their own order, neighbour tables of 1, 4 and 8 groups.  Per tile of 32
    consecutive rows (coarse_sets with eps_m = filter_eps + filter_rho: the walk over the means keeps hi*hi only): the
    id is live and lies in a group of the upper set U; true_dist(id) <= the smallest true distance among the
    centroids of the lower set L + 2 filter_eps; |dist - true_dist(id)| <= filter_eps; nothing is written behind
    row n."""
    seed, nsuper = gr.COARSE_TABLES[(d, k)]
    key = ("origin", d, k, seed, nsuper)
    x, c = gr.table(*key)
    dead = _coarse_case(be, key, x[:n], c, gr.truth(*key)[:n], _kd(be, key, c), f"coarse d={d} n={n} k={k}")
    assert dead == 0


@pytest.mark.parametrize("d,n,k", gr.COARSE_PADDED_CASES)
def test_coarse_pass_on_the_padded_grouping(be, d, n, k):
    """The same on the hand-made grouping: padding slots in the middle of every group, and a group of padding only
    whose mean, the zero vector, sits in the means image like any other.  The neighbour tables of 4 and 8 groups name
    it in every tile (the origin is nearer to a super-centre than most other super-centres are), so the second walk
    meets a group whose 32 slots all read |c|^2 = +inf beside live ones.  The last row is the zero row, which names that
    group; at n = 129 it is alone in its tile and, under the table of one neighbour, has nothing live to search: the
    answer there is -1 with dist = +inf (asserted to occur), and an id everywhere else."""
    key, x, c, T = gr.coarse_padded_inputs(d, n, k)
    dead = _coarse_case(be, key, x, c, T, gr.kd_padded_cperm(_kd(be, key, c)), f"coarse padded d={d} n={n} k={k}")
    assert dead == (1 if n % 32 == 1 else 0)


# ---------------------------------------------------------------------------------------------------------------------
# (g) across calls

@pytest.mark.parametrize("d", [64, 128])
def test_coarse_pass_between_other_calls(be, oracle, d):
    """The coarse pass at k = 1285, then at k = 16384 (the two fp16 images and the identity grouping of the means
    grow), then group_min_dist + assign_pruned(image_current=True) on the first table: the oracle's bits; then
    group_min_dist, a coarse pass over the OTHER table and only then assign_pruned(image_current=True): the coarse pass
    has overwritten the image that group_min_dist left and withdrawn it, so the sweep must rebuild it -- the oracle's
    bits again; then the first coarse call once more: the ids and distances of its first run."""
    tabs = {}
    for k in (1285, 16384):
        seed, nsuper = gr.COARSE_TABLES[(d, k)]
        key = ("origin", d, k, seed, nsuper)
        x, c = gr.table(*key)
        xt, ct, cperm = _dev(be, x), _dev(be, c), _dev(be, _kd(be, key, c))
        means = be.group_means(ct, cperm)
        tabs[k] = (key, x, c, xt, ct, cperm, means, be.group_neighbours(means, 4))
    key, x, c, xt, ct, cperm, means, gnbr = tabs[1285]
    _, _, _, xt2, ct2, cperm2, means2, gnbr2 = tabs[16384]
    ids_o, dis_o = _oracle(oracle, key, x, c)
    first = [t.cpu().numpy() for t in be.assign_coarse(xt, ct, cperm, means, gnbr)]
    be.assign_coarse(xt2, ct2, cperm2, means2, gnbr2)
    order = be.visit_order(_dev(be, first[0]), _dev(be, first[1]), 1285)
    for between in (False, True):
        dmin = be.group_min_dist(ct, cperm)
        if between:
            be.assign_coarse(xt2, ct2, cperm2, means2, gnbr2)
        ids, dis = be.assign_pruned(xt, ct, order, cperm, dmin, filter=True, image_current=True)
        assert np.array_equal(ids.cpu().numpy(), ids_o), f"coarse pass in between: {between}"
        assert np.array_equal(bits(dis.cpu().numpy()), bits(dis_o)), f"coarse pass in between: {between}"
    again = [t.cpu().numpy() for t in be.assign_coarse(xt, ct, cperm, means, gnbr)]
    assert np.array_equal(again[0], first[0]) and np.array_equal(bits(again[1]), bits(first[1]))
