"""The seams of the fp32 MFMA sweeps of assign.hip: partial last tiles and partial last workgroups on every launched
instantiation, bit for bit against oracle.assign.

The five sweeps share their load and store steps (assign.hip, "The steps that the MFMA sweeps below share").  What such
a step can get wrong shows where a launch ends: a row tile of fewer than 32 rows (rows past n are clamped on the way in
and must not be stored on the way out), a wave or a workgroup with no row at all, a last centroid tile or group that is
partly padding.  The other tests run these kernels at a handful of sizes; here every instantiation a route or an A/B
switch can launch runs at every n of NS: one row more and one row fewer than 1, 2, 4 and 8 tiles of 32 rows, the
smallest n of the MFMA routes (20), and 513 (more than one workgroup of every geometry: a workgroup holds 32 to 512
rows).  k = 300 leaves the last 128- and 64-centroid tile of the dense and hinted sweeps partly empty, k = 1000 the
last 32-centroid group of the pruned ones.

Data: seeded clustered unit rows; ten centroids duplicated at higher indices with rows sitting exactly on them (the
lowest index must win the tie on every route); one row whose squared norm overflows, which is (-1, +inf) on every
route whatever it was hinted.  The reference is computed once per (d, k) for the 513 rows; a case takes its first n.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (20, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
N_MAX = max(NS)
OVERFLOW_ROW = 7                    # inside the first 20 rows, so that every n has it
TIE_ROWS = np.arange(10, 20)        # rows that sit on the duplicated centroids 0 .. 9
_CASES = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _case(be, oracle, d, k):
    """x [513, d], c [k, d] with the oracle's answer and an 80 %-right guess per row: built once, shared, read-only."""
    key = (d, k)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * d + k)
        centers = oracle.l2norm_rows(rng.standard_normal((k, d)).astype(np.float32))
        x = oracle.l2norm_rows((centers[rng.integers(0, k, N_MAX)] + 0.05 * rng.standard_normal((N_MAX, d))).astype(np.float32))
        c = oracle.l2norm_rows((centers + 0.01 * rng.standard_normal((k, d))).astype(np.float32))
        c[k - 100:k - 90] = c[0:10]
        x[TIE_ROWS] = c[0:10]
        x[OVERFLOW_ROW] = np.float32(1e19)          # finite elements, |x|^2 = d * 1e38 = +inf
        ids, dis = oracle.assign(x, c)
        assert ids[OVERFLOW_ROW] == -1 and np.isposinf(dis[OVERFLOW_ROW])
        assert np.array_equal(ids[TIE_ROWS], np.arange(10)) and (dis[TIE_ROWS] < 1e-6).all()
        random = rng.integers(0, k, N_MAX)
        guess = np.where((rng.random(N_MAX) < 0.8) & (ids >= 0), ids, random)
        case = dict(x=x, c=c, ids=ids, dis=dis, guess=guess, random=random)
        if d in (64, 128):
            case["cperm"] = be.group_rows_kd(c)
        for v in case.values():
            v.setflags(write=False)
        _CASES[key] = case
    return _CASES[key]


def _same(got, case, n, what):
    ids, dis = got
    ids, dis = ids.cpu().numpy(), dis.cpu().numpy()
    assert ids.shape == (n,) and dis.shape == (n,), what
    bad = np.nonzero(ids != case["ids"][:n])[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {n} ids differ, first at row {bad[0]}: got {ids[bad[0]]} want "
                           f"{case['ids'][bad[0]]}")
    bad = np.nonzero(bits(dis) != bits(case["dis"][:n]))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {n} distances differ, first at row {bad[0]}: got {dis[bad[0]]!r} want "
                           f"{case['dis'][bad[0]]!r}")
    assert ids[OVERFLOW_ROW] == -1 and np.isposinf(dis[OVERFLOW_ROW]), what


@pytest.mark.parametrize("variant", [0, 1, 3])
@pytest.mark.parametrize("d", [64, 128])
def test_dense_sweep(be, oracle, switches, d, variant):
    """be.assign at d = 64 / 128: the shipped LDS-DMA kernel, the register-staged one (1) and the speculative
    epilogue (3)."""
    case = _case(be, oracle, d, 300)
    switches(assign_variant=variant)
    xt, ct = be._f32(case["x"]), be._f32(case["c"])
    for n in NS:
        _same(be.assign(xt[:n], ct), case, n, f"assign d={d} assign_variant={variant} n={n}")


@pytest.mark.parametrize("variant", [0, 4, 5, 6])
@pytest.mark.parametrize("d", [192, 68])
def test_anyd_sweep(be, oracle, switches, d, variant):
    """be.assign through the chunked sweep, three whole chunks (192) and a padded last chunk (68), in its four shapes."""
    case = _case(be, oracle, d, 300)
    switches(assign_variant=variant)
    xt, ct = be._f32(case["x"]), be._f32(case["c"])
    for n in NS:
        _same(be.assign(xt[:n], ct), case, n, f"assign d={d} assign_variant={variant} n={n}")


@pytest.mark.parametrize("d", [64, 128])
def test_hinted_sweep(be, oracle, d):
    """be.assign_hinted with the right guesses, random ones and none, in row order and in member-list order."""
    k = 300
    case = _case(be, oracle, d, k)
    xt, ct = be._f32(case["x"]), be._f32(case["c"])
    hints = {"right": case["ids"], "random": case["random"], "none": np.full(N_MAX, -1, np.int64)}
    for n in NS:
        for hname, hint in hints.items():
            hint = torch.from_numpy(np.ascontiguousarray(hint[:n], dtype=np.int64)).to(be.device)
            _, member_order = be.centroid_accum(xt[:n], torch.clamp(hint, min=0, max=k - 1), k, want_order=True)
            for oname, order in (("row order", None), ("member-list order", member_order)):
                _same(be.assign_hinted(xt[:n], ct, hint, order), case, n, f"assign_hinted d={d} hint={hname} {oname} n={n}")


def _pruned(be, case, k, d, n, what):
    xt, ct = be._f32(case["x"][:n]), be._f32(case["c"])
    cperm = be.from_host(case["cperm"])
    dmin = be.group_min_dist(ct, cperm)
    guess = torch.from_numpy(np.ascontiguousarray(case["guess"][:n])).to(be.device)
    order = be.visit_order(guess, None, k)
    _same(be.assign_pruned(xt, ct, order, cperm, dmin, filter=False), case, n, what)


@pytest.mark.parametrize("prune_kernel", [1, 0])
@pytest.mark.parametrize("prune_nb", [0, 1, 4])
def test_pruned_sweep_d64(be, oracle, switches, prune_nb, prune_kernel):
    """be.assign_pruned(filter=False) at d = 64: one, two and four row tiles per wave, in the register-staged form
    (prune_kernel = 1; four tiles exist in the LDS-DMA form only) and in the LDS-DMA form."""
    case = _case(be, oracle, 64, 1000)
    switches(prune_nb=prune_nb, prune_kernel=prune_kernel)
    for n in NS:
        _pruned(be, case, 1000, 64, n, f"assign_pruned d=64 prune_nb={prune_nb} prune_kernel={prune_kernel} n={n}")


def test_pruned_sweep_d128(be, oracle):
    """be.assign_pruned(filter=False) at d = 128: the LDS-DMA form, two row tiles per wave."""
    case = _case(be, oracle, 128, 1000)
    for n in NS:
        _pruned(be, case, 1000, 128, n, f"assign_pruned d=128 n={n}")
