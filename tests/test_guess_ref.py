"""The float64 models of tests/guess_ref.py against brute force, and the conditions that keep tests/test_gpu_guesses.py
from passing vacuously, on the very inputs it uses.  No GPU.

Conditions (caps set beforehand; the values found are in DESIGN.md section 5.0d):
    pre-pass masks   on every (rung, d, n, k) of guess_ref.MASK_CASES the pairs that mask_bracket leaves undecided
                     (may & ~must) are at most 0.5 % of the `must` pairs, with a device dmin modelled as the true one
                     x (1 - 2e-5); on origin and db `must` sets between 20 % and 80 % of all pairs.
    coarse pass      on every (d, n, k) of guess_ref.COARSE_CASES at most 1 % of the rows have more than one
                     admissible nearest mean and no tile has an empty lower set.  On the hand-made grouping
                     (COARSE_PADDED_CASES) the same, and: the zero mean of the group of padding only is admissible for
                     the planted zero row alone; every tile's lower set has a live member, except the one-row tile of
                     the zero row under a table of one neighbour, whose sets are that group alone (-1 is due there)."""
import numpy as np
import pytest

import guess_ref as gr
import off_origin_data as od
from audio_tokens_amd.backend import HostHelpers

_HOST = {}


def _kd(c):
    if "h" not in _HOST:
        _HOST["h"] = HostHelpers()
    return _HOST["h"].group_rows_kd(c)


# ---- models against brute force -------------------------------------------------------------------------------------
def test_bit_tables_round_trip():
    rng = np.random.default_rng(0)
    b = rng.random((5, 70)) < 0.3
    w = gr.bool_to_bits(b)
    assert w.shape == (5, 3) and w.dtype == np.uint32
    back = gr.bits_to_bool(w, 70)
    assert back.shape == (5, 96) and np.array_equal(back[:, :70], b) and not back[:, 70:].any()
    assert gr.bits_to_bool(np.array([[0x80000001]], np.uint32).view(np.int32), 32)[0].nonzero()[0].tolist() == [0, 31]


def test_group_means_model_by_hand():
    c = np.array([[1.0, 2.0], [3.0, 5.0], [1e8, 1.0], [0.5, -1.0]], np.float32)
    cperm = np.full(96, -1, np.int32)
    cperm[[0, 5]] = [1, 0]             # group 0: rows 1, 0 with padding between them
    cperm[[33, 40, 63]] = [2, 3, 0]    # group 1: 1e8 + 0.5 rounds to 1e8 in fp32, then + 1
    means = gr.group_means_model(c, cperm)
    assert means.dtype == np.float32 and means.shape == (3, 2)
    assert np.array_equal(means[0], np.array([2.0, 3.5], np.float32))
    want = (np.float32(np.float32(1e8) + np.float32(0.5)) + np.float32(1.0)) / np.float32(3.0)
    assert means[1, 0] == want and means[1, 1] == np.float32(2.0) / np.float32(3.0)
    assert np.array_equal(means[2], np.zeros(2, np.float32))       # padding only


def test_tile_candidates_by_hand():
    """Three groups, 40 positions: tile 0 names groups 0 and 2, tile 1 (8 positions) names group 1 and one row names
    no group at all."""
    g = np.array([0] * 20 + [2] * 12 + [1] * 7 + [3])
    got = gr.tile_candidates(g, None, 3)
    assert got.tolist() == [[True, False, True], [False, True, False]]
    gnbr = np.array([[0b011], [0b010], [0b110]], np.uint32)          # 0 -> {0, 1}, 1 -> {1}, 2 -> {1, 2}
    got = gr.tile_candidates(g, gnbr, 3)
    assert got.tolist() == [[True, True, True], [False, True, False]]
    brute = np.zeros((2, 3), bool)
    for i, gi in enumerate(g):
        for h in range(3):
            if gi < 3 and (gnbr[gi, 0] >> h) & 1:
                brute[i // 32, h] = True
    assert np.array_equal(got, brute)


def test_coarse_sets_by_hand():
    """Three means on a line at 0, 10 and 11; rows at 1 (nearest mean 0, alone), at 10.5 (means 1 and 2 tie) and at
    10.4 (mean 1 wins by 0.2: alone at eps 0.05, ambiguous at eps 0.2)."""
    means = np.array([[0.0], [10.0], [11.0]])
    gnbr = np.array([[0b001], [0b011], [0b100]], np.uint32)          # 0 -> {0}, 1 -> {0, 1}, 2 -> {2}
    x = np.array([[1.0]] * 32 + [[10.5], [10.4]])
    L, U, adm = gr.coarse_sets(x, means, gnbr, np.full(34, 0.05))
    assert adm[0].tolist() == [True, False, False] and adm[32].tolist() == [False, True, True]
    assert adm[33].tolist() == [False, True, False]
    assert L.tolist() == [[True, False, False], [True, True, False]]
    assert U.tolist() == [[True, False, False], [True, True, True]]
    L, U, adm = gr.coarse_sets(x, means, gnbr, np.full(34, 0.2))
    assert adm[33].tolist() == [False, True, True]
    assert L.tolist() == [[True, False, False], [False, False, False]]      # tile 1: no row is sure of its mean
    assert U.tolist() == [[True, False, False], [True, True, True]]


def test_mask_bracket_by_hand():
    """Two tiles, d = 64, three groups.  Tile 0 holds two runs: guess 0 (radius 2 sqrt(1) = 2) and guess 1 (radius
    2 sqrt(4) = 4); tile 1 holds guess 0 at radius 2 and, in a second case, a row without a guess."""
    d = 64
    dmin = np.array([[0.0, 1.9, 4.5], [3.9, 0.0, 4.0001], [9.0, 9.0, 0.0]])
    p = np.array([0] * 16 + [1] * 16 + [0] * 3)
    bd = np.array([1.0] * 16 + [4.0] * 16 + [1.0] * 3)
    has = np.ones(35, bool)
    xn = np.zeros(35)
    must, may = gr.mask_bracket(bd, p, has, dmin, xn, 0.0, d)
    # 4.0001 against tau = 4: inside neither (margin 1e-4 makes it 4.0004 for `may`: inside)
    assert must.tolist() == [[True, True, False], [True, True, False]]
    assert may.tolist() == [[True, True, True], [True, True, False]]
    for factor, got in ((1 - gr.MARGIN, must), (1 + gr.MARGIN, may)):
        assert np.array_equal(got, gr.mask_brute(bd, p, has, dmin, xn, 0.0, d, factor))
    # delta: |x|^2 + max|c|^2 = 1e6 adds 1.01 * 136 * 2^-24 * 1e6 = 8.19 under the root: tau = 2 sqrt(9.19) = 6.06
    must, may = gr.mask_bracket(bd, p, has, dmin, xn + 1e6, 0.0, d)
    assert must.tolist() == [[True, True, True], [True, True, True]]
    must, may = gr.mask_bracket(bd, p, has, dmin, xn, 0.0, d)
    has2 = has.copy()
    has2[34] = False
    bd2 = bd.copy()
    bd2[34] = np.inf
    p2 = p.copy()
    p2[34] = 3                     # (what hint_sorted holds for a row without a guess: k)
    must, may = gr.mask_bracket(bd2, p2, has2, dmin, xn, 0.0, d)
    assert must.tolist() == [[True, True, False], [True, True, True]] and may[1].all()
    assert np.array_equal(must, gr.mask_brute(bd2, p2, has2, dmin, xn, 0.0, d, 1 - gr.MARGIN))


def test_visit_order_model_by_hand():
    ids = np.array([2, -1, 0, 2, 0, 7])
    dis = np.array([4.0, 0.0, 1.0, 0.01, 1.0, 0.0], np.float32)
    order, hs = gr.visit_order_model(ids, dis, 3)
    assert order.tolist() == [2, 4, 3, 0, 1, 5] and hs.tolist() == [0, 0, 2, 2, 3, 3]


def test_filter_bounds_match_the_source_constants():
    """filter_eps is the header of csrc/filter.hip; dmin_f16_bound is eps_a H' + eps_b of at_group_min_dist_f16, which
    is eps (x 1.001, with the 1.0001 of filter_tau) + rho: a little above filter_eps + filter_rho, never below."""
    for d in (64, 128):
        for H in (1.0, 140.0, 1.3e6):
            lo = gr.filter_eps(d, H) + gr.filter_rho(d, H)
            got = gr.dmin_f16_bound(d, H / 2 / 1.001, H / 2)
            assert lo <= got <= lo * 1.002
            assert gr.filter_eps(d, H) <= gr.dmin_f16_bound(d, H / 2 / 1.001, H / 2, three=True) <= gr.filter_eps(d, H) * 1.002


# ---- the conditions on the inputs of the GPU tests ----------------------------------------------------------------------
@pytest.mark.parametrize("name,d,n,k,none_tail", gr.MASK_CASES)
def test_mask_inputs_decide_and_prune(name, d, n, k, none_tail):
    m = gr.mask_inputs(name, d, n, k, none_tail)
    cperm = _kd(m["c"])
    ng = cperm.size // 32
    assert ng == gr.GROUPS[k]
    hs, has, order = m["hs"], m["has"], m["order"]
    if none_tail is not None:
        assert (~has).sum() == none_tail and not has[n - none_tail:].any() and (n - none_tail) % 32 in (0, 16)
    else:
        assert (~has).sum() == n // 37
    guessed = np.unique(hs[has])
    dmin = np.zeros((k, ng))
    dmin[guessed] = gr.group_min_rows(m["c"], cperm, guessed) * (1.0 - 2e-5)
    bd = np.where(has, m["T"][order, np.where(has, hs, 0)], np.inf)
    must, may = gr.mask_bracket(bd, hs, has, dmin, gr.sq_norms(m["x"][order]), gr.sq_norms(m["c"]).max(), d)
    assert must.shape == ((n + 31) // 32, ng)
    undecided = int((may & ~must).sum())
    print(f"\nMEASURE {name} d={d} n={n} k={k} none_tail={none_tail}: must {must.sum()} of {must.size} "
          f"({must.mean():.3f}), undecided {undecided}")
    assert not (must & ~may).any()
    assert undecided <= 0.005 * must.sum()
    if name in gr.BAND_RUNGS:
        assert 0.2 <= must.mean() <= 0.8
    else:
        assert 0 < must.sum() < must.size
    # the tiles hold several runs, and a second-nearest guess is among them
    runs = [np.unique(hs[t:t + 32]).size for t in range(0, n, 32)]
    assert max(runs) >= 2
    assert (m["ids"][m["ids"] >= 0] != m["T"].argmin(axis=1)[m["ids"] >= 0]).any()


@pytest.mark.parametrize("d,n,k", gr.COARSE_CASES)
def test_coarse_inputs_are_decided(d, n, k):
    seed, nsuper = gr.COARSE_TABLES[(d, k)]
    x, c = gr.table("origin", d, k, seed, nsuper)
    x = x[:n]
    cperm = _kd(c)
    ng = cperm.size // 32
    assert ng == gr.GROUPS[k]
    means = gr.group_means_model(c, cperm)
    eps, eps_m = gr.coarse_eps(d, x, c)
    L, U, adm = gr.coarse_sets(x, means, gr.group_neighbours_model(means, 4), eps_m)
    ambiguous = int((adm.sum(axis=1) > 1).sum())
    T = np.sort(od.true_sqdist(x, means), axis=1)
    print(f"\nMEASURE coarse d={d} n={n} k={k}: ambiguous rows {ambiguous} of {n}, median best-to-second gap of the "
          f"means {np.median((T[:, 1] - T[:, 0]) / eps_m):.0f} eps_m, L sets {L.mean():.3f} U sets {U.mean():.3f} of the pairs")
    assert ambiguous <= 0.01 * n
    assert L.any(axis=1).all()
    assert not (L & ~U).any()


@pytest.mark.parametrize("d,n,k", gr.COARSE_PADDED_CASES)
def test_coarse_inputs_on_the_padded_grouping(d, n, k):
    key, x, c, T = gr.coarse_padded_inputs(d, n, k)
    cperm = gr.kd_padded_cperm(_kd(c))
    ng = cperm.size // 32
    own = gr.group_of(cperm, k)
    live = np.bincount(own, minlength=ng) > 0
    assert ng == 44 and live[:-1].all() and not live[-1]
    means = gr.group_means_model(c, cperm)
    assert not means[-1].any()
    eps, eps_m = gr.coarse_eps(d, x, c)
    for nnb in (1, 4, 8):
        gnbr = gr.group_neighbours_model(means, nnb)
        L, U, adm = gr.coarse_sets(x, means, gnbr, eps_m)
        ambiguous = int((adm.sum(axis=1) > 1).sum())
        assert ambiguous <= 0.01 * n
        assert np.nonzero(adm[:, -1])[0].tolist() == [n - 1] and adm[n - 1].sum() == 1
        assert L.any(axis=1).all()
        dead = np.nonzero(~(L & live).any(axis=1))[0].tolist()
        lone = n % 32 == 1 and nnb == 1
        assert dead == ([(n - 1) // 32] if lone else [])
        if lone:
            assert not (U[-1] & live).any()
        print(f"\nMEASURE coarse padded d={d} n={n} nnb={nnb}: ambiguous rows {ambiguous} of {n}; the group of padding "
              f"only is in L of {int(L[:, -1].sum())} of {L.shape[0]} tiles")
