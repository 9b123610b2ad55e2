"""The off-origin ladder (tests/off_origin_data.py) is what it claims to be -- the oracle and float64 only, no GPU.

tests/test_gpu_off_origin.py holds every exact nearest-centroid route to the oracle on these rungs; that proves
something only if the rungs really load the margins they are named for.  Here, at n = 4129, k = 1000, d in (64, 128):
how often the fp32 contract's winner is not the float64 winner, how many rows sit at distance 0, how wide the ties at
0 are, and how much the Elkan rule could skip with exact centroid distances and the contract's radius.

The contract's whole distance matrix comes from the oracle itself, one call per centroid column (knn_ref.distance_matrix);
its row-wise lowest-index arg-min must be oracle.assign's answer on every row, so the matrix is never trusted blindly.

Measured (seed 9), d = 64 / 128:
    rung    contract != fp64    rows at 0        Elkan share     widest tie at 0   distinct winners
    origin  0      / 0          .0048 / .0048    .980 / .981     2   / 2           968 / 967
    far     .0007  / .0002      .0048 / .0048    .951 / .981     2   / 2
    edge    .0015  / .0007      .0048 / .0048    .305 / .103     2   / 2
    clamp   .0107  / .0116      .197  / .272     0    / 0        2   / 2
    wrong   .0465  / .1458      .505  / .497     0    / 0        3   / 8
    flat    .9981  / .9988      1.0   / 1.0      0    / 0        974 / 944         22  / 23
    db      0      / 0          .0048 / .0048    .979 / .981     2   / 2
max |computed - true| / delta over all pairs: at most 0.104 (the bound of csrc/prune.hip holds with room)."""
import numpy as np
import pytest

import off_origin_data as od
from knn_ref import distance_matrix

_CACHE = {}


def _rung_facts(oracle, name, d):
    """Computed once per (rung, d) and shared, never modified."""
    key = (name, d)
    if key not in _CACHE:
        x, c = od.rung(name, d)
        ids, dis = oracle.assign(x, c)
        D, ok = distance_matrix(oracle, x, c)
        assert ok.all()
        f = od.facts(x, c)
        for a in (x, c, ids, dis, D, f["T"], f["arg"]):
            a.setflags(write=False)
        _CACHE[key] = (x, c, ids, dis, D, f)
    return _CACHE[key]


CASES = [(name, d) for d in (64, 128) for name in od.RUNG_NAMES]


@pytest.mark.parametrize("name,d", CASES)
def test_the_contract_matrix_is_the_oracles(oracle, name, d):
    """Row-wise lowest-index arg-min and minimum of the column-by-column matrix == oracle.assign, bit for bit, on every
    row; and every computed distance is within delta = (2d + 8) u (|x|^2 + max|c|^2) of the float64 one."""
    x, c, ids, dis, D, f = _rung_facts(oracle, name, d)
    assert x.shape == (od.N, d) and c.shape == (od.K, d) and x.dtype == np.float32 and c.dtype == np.float32
    assert np.array_equal(D.argmin(axis=1), ids)
    assert np.array_equal(D.min(axis=1).view(np.uint32), dis.view(np.uint32))
    ratio = (np.abs(D.astype(np.float64) - f["T"]) / od.delta_bound(x, c)[:, None]).max()
    print(f"\nMEASURE {name} d={d}: max |computed - true| / delta = {ratio:.3f}")
    assert ratio <= 1.0


def test_true_distances_come_from_differences(oracle):
    """The float64 reference itself: cdist's non-matmul mode against the plain numpy sum of squared differences."""
    x, c = od.rung("flat", 64)
    T = od.true_sqdist(x[:50], c)
    ref = ((x[:50, None, :].astype(np.float64) - c[None, :, :].astype(np.float64)) ** 2).sum(-1)
    assert np.allclose(T, ref, rtol=1e-14, atol=0)
    assert np.array_equal(T[:20].argmin(1), np.arange(20)) and (T[np.arange(20), np.arange(20)] == 0).all()
    assert np.allclose(od.true_rowwise_sqdist(x[:50], c[:50]), ref[np.arange(50), np.arange(50)], rtol=1e-14, atol=0)
    cperm = np.full(od.K // 32 * 32 + 64, -1, np.int32)            # 33 groups: the last one padding only
    cperm[:od.K] = np.random.default_rng(1).permutation(od.K)
    gmin = od.true_group_min(c, cperm)
    assert gmin.shape == (od.K, 33) and np.isinf(gmin[:, 32]).all() and np.isfinite(gmin[:, :32]).all()
    g, m = 5, cperm[5 * 32: 6 * 32]
    cc = np.sqrt(((c[:, None, :].astype(np.float64) - c[None, m, :].astype(np.float64)) ** 2).sum(-1)).min(1)
    assert np.allclose(gmin[:, g], cc, rtol=1e-14, atol=0)


@pytest.mark.parametrize("name,d", CASES)
def test_rung_regime(oracle, name, d):
    x, c, ids, dis, D, f = _rung_facts(oracle, name, d)
    neq = float((ids != f["arg"]).mean())
    zero = float((dis == 0).mean())
    zeros_per_row = (D == 0).sum(axis=1)
    print(f"\nMEASURE {name} d={d}: contract != fp64 {neq:.4f}, rows at 0 {zero:.4f}, widest tie at 0 "
          f"{zeros_per_row.max()}, distinct winners {np.unique(ids).size}")
    # the 20 planted duplicates: at distance 0 whatever the offset, and never the higher twin
    assert (ids[:20] <= np.arange(20)).all() and (dis[:20] == 0).all()
    if name in ("origin", "db"):
        assert neq == 0 and zero <= 0.01
    elif name in ("far", "edge"):
        assert neq <= 0.01 and zero <= 0.01
    elif name == "clamp":
        assert neq > 0 and 0.1 <= zero <= 0.4
    elif name == "wrong":
        assert neq >= 0.02 and zero >= 0.4
    else:
        assert name == "flat"
        assert neq >= 0.9 and zero == 1.0
        assert zeros_per_row.max() >= 500
        assert np.unique(ids).size < 64
        assert np.array_equal(ids, (D == 0).argmax(axis=1))      # the lowest index among the row's zeros


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", ["far", "edge"])
def test_elkan_share_in_exact_arithmetic(oracle, name, d):
    """What Elkan's rule could skip with p = the contract's winner, R^2 = dis + delta and exact centroid distances:
    the share of (row, centroid) pairs with |c - c_p| > 2 R.  `far` still prunes nearly everything, `edge` a part."""
    x, c, ids, dis, D, f = _rung_facts(oracle, name, d)
    R = np.sqrt(dis.astype(np.float64) + od.delta_bound(x, c))
    cc = np.sqrt(od.true_sqdist(c, c))
    share = float((cc[ids] > 2.0 * R[:, None]).mean())
    print(f"\nMEASURE {name} d={d}: Elkan share {share:.3f}")
    if name == "far":
        assert share > 0.9
    else:
        assert 0.03 < share < 0.5
