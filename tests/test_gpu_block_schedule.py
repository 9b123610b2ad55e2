"""The block schedules of the exact filter sweep on the device (csrc/prune.hip makes them beside the visiting order,
csrc/filter.hip starts its row blocks by them, csrc/exact_search.cpp decides which sweep may): the tables against the
numpy model (block_schedule_ref.py), the results under every block order against the oracle, and the tag that keeps a
table away from sweeps it was not made for."""
import numpy as np
import pytest
import torch

import block_schedule_ref as bs
import guess_ref as gr

pytestmark = pytest.mark.gpu
K = 1285


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture()
def sched(be, switches):
    """The defaults of the schedule switches, before and after."""
    be.block_sched_install(None)
    be.debug_set("block_sched", 1)
    yield switches
    be.block_sched_install(None)
    be.debug_set("block_sched", 1)


def _dev(be, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(be.device).contiguous()


def _check_tables(be, ids, dis, k, what):
    order = be.visit_order(_dev(be, ids, torch.int64), None if dis is None else _dev(be, dis, torch.float32), k)
    keys = np.sort(bs.make_keys(ids, dis, k))
    w = bs.tile_weights(keys, k)
    for tiles in (1, 2, 4):
        table, weight = be.block_sched_peek(order[0], tiles)
        assert np.array_equal(weight.cpu().numpy(), w), f"{what}: tile weights"
        table = table.cpu().numpy().view(np.uint32).astype(np.int64)
        assert table.size == -(-w.size // tiles)
        assert bs.is_schedule_of(table, bs.block_classes(w, tiles)), f"{what}, {tiles} tiles: not a schedule of its classes"
        assert np.array_equal(table, bs.schedule(w, tiles)), f"{what}, {tiles} tiles"


@pytest.mark.parametrize("k", [33, K])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4097])
def test_tables_are_the_models(be, sched, n, k):
    """With and without distances, with a tail of rows without a guess, and with every row in one cluster."""
    rng = np.random.default_rng(n * 7 + k)
    ids = rng.integers(0, k, n)
    dis = (rng.random(n) ** 2 * 1.5).astype(np.float32)
    dis[rng.random(n) < 0.02] = 5.0                       # beyond the range of the distance field
    _check_tables(be, ids, dis, k, "distances")
    _check_tables(be, ids, None, k, "no distances")
    tail = ids.copy()
    tail[n - max(1, n // 5):] = -1
    _check_tables(be, tail, dis, k, "tail without a guess")
    _check_tables(be, np.full(n, 7), dis, k, "one cluster")


@pytest.mark.parametrize("which,delta", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_tables_on_both_sides_of_a_change_of_block_size(be, sched, which, delta):
    """The row counts at which the sweep goes from one tile per block to two and from two to four (read from the plan):
    more than one workgroup of the counting sort, and a last chunk that is not full."""
    n = be.block_sched_limits()[which] + delta
    rng = np.random.default_rng(which * 2 + delta)
    ids = rng.integers(0, K, n)
    ids[rng.random(n) < 0.001] = -1
    dis = (rng.random(n).astype(np.float32) ** 2 * np.float32(1.5))
    _check_tables(be, ids, dis, K, f"n={n}")


# ---- results -----------------------------------------------------------------------------------------------------------
_CASE = {}


def _case(be, oracle, d):
    """x [2033, d] (63 tiles and 17 rows: no multiple of any block), c [1285, d] with 20 duplicated centroids and the
    rows that sit on them (ties: listed for the redo), the oracle's answer and guesses that are right for 4 rows in 5."""
    if d not in _CASE:
        x, c = (np.array(a) for a in gr.table("origin", d, K))
        c[K // 2:K // 2 + 20] = c[0:20]
        x[:20] = c[0:20]
        ids_o, dis_o = oracle.assign(x, c)
        rng = np.random.default_rng(d)
        guess = np.where(rng.random(x.shape[0]) < 0.2, rng.integers(0, K, x.shape[0]), ids_o)
        guess[np.arange(x.shape[0]) % 37 == 36] = -1
        ct = be._f32(c)
        cperm = be.from_host(be.group_rows_kd(c))
        _CASE[d] = dict(x=be._f32(x), c=ct, cperm=cperm, dmin=be.group_min_dist(ct, cperm), ids_o=ids_o, dis_o=dis_o,
                        guess=_dev(be, guess, torch.int64), gdis=_dev(be, dis_o, torch.float32), guess_host=guess)
    return _CASE[d]


def _sweep(be, case, order, path, what, tiles=None):
    ids, dis = be.assign_pruned(case["x"], case["c"], order, case["cperm"], case["dmin"], filter=True)
    ids, dis = ids.cpu().numpy(), dis.cpu().numpy()
    got = be.block_sched_last()
    assert got[0] == path, f"{what}: path {got[0]}, not {path}"
    if tiles:
        assert got[1] == tiles and got[2] == -(-case["x"].shape[0] // (32 * tiles)), f"{what}: {got}"
    assert np.array_equal(ids, case["ids_o"]), f"{what}: {(ids != case['ids_o']).sum()} ids differ"
    assert np.array_equal(bits(dis), bits(case["dis_o"])), f"{what}: distances differ"
    return got


@pytest.mark.parametrize("sync", [0, 1])
@pytest.mark.parametrize("d,nb", [(64, 1), (64, 2), (64, 4), (128, 0)])
def test_every_block_order_gives_the_oracles_result(be, oracle, sched, d, nb, sync):
    case = _case(be, oracle, d)
    sched(filter_nb=nb, filter_sync=sync)
    tiles = nb or 2
    order = be.visit_order(case["guess"], case["gdis"], K)
    be.filter_stats(reset=True)
    blocks = _sweep(be, case, order, 1, "schedule on", tiles)[2]
    rows, listed = be.filter_stats()
    assert rows == case["x"].shape[0] and listed >= 20            # the tied rows go through the redo
    be.debug_set("block_sched", 0)
    _sweep(be, case, order, 0, "schedule off", tiles)
    rng = np.random.default_rng(d + nb)
    for name, table in (("reversed", np.arange(blocks)[::-1]), ("random", rng.permutation(blocks))):
        be.block_sched_install(table)
        _sweep(be, case, order, 2, f"{name} schedule installed", tiles)
    be.block_sched_install(None)
    _sweep(be, case, order, 0, "installed schedule removed", tiles)


def test_install_refuses_what_is_no_permutation(be, sched):
    for bad in ([0, 1, 1], [0, 1, 3], [2, 2, 2]):
        with pytest.raises(RuntimeError, match="not a permutation"):
            be.block_sched_install(bad)


# ---- the tag -----------------------------------------------------------------------------------------------------------
def test_a_table_serves_only_the_order_it_was_made_beside(be, oracle, sched):
    from audio_tokens_amd import _lib
    from audio_tokens_amd.backend import HipBackend
    case = _case(be, oracle, 64)
    n = case["x"].shape[0]
    order = be.visit_order(case["guess"], case["gdis"], K)
    _sweep(be, case, order, 1, "the order of the last visit_order")
    # a host-made order of the same n at another address
    order_h, hs_h = gr.visit_order_model(case["guess_host"], case["dis_o"], K)
    host_made = (_dev(be, order_h, torch.int32), _dev(be, hs_h, torch.int32))
    _sweep(be, case, host_made, 0, "host-made order, same n")
    # the returned tensors overwritten in place with another permutation: still a schedule of its blocks
    other = np.where(np.arange(n) % 3 == 0, (case["guess_host"] + 5) % K, case["guess_host"])
    order_o, hs_o = gr.visit_order_model(other, None, K)
    order[0].copy_(_dev(be, order_o, torch.int32))
    order[1].copy_(_dev(be, hs_o, torch.int32))
    _sweep(be, case, order, 1, "order overwritten in place")
    # a visit order of another n lays the tables out anew: the earlier order goes back to the visiting order
    short = be.visit_order(case["guess"][:1000].contiguous(), case["gdis"][:1000].contiguous(), K)
    assert be.block_sched_peek(short[0], 1) is not None and be.block_sched_peek(order[0], 1) is None
    _sweep(be, case, order, 0, "after a visit_order of another n")
    # two in a row: both halves hold a table
    first = be.visit_order(case["guess"], case["gdis"], K)
    second = be.visit_order(_dev(be, other, torch.int64), None, K)
    assert be.block_sched_peek(first[0], 2) is not None and be.block_sched_peek(second[0], 2) is not None
    _sweep(be, case, first, 1, "first of two visit orders")
    _sweep(be, case, second, 1, "second of two visit orders")
    _sweep(be, case, first, 1, "first of two visit orders, again")
    third = be.visit_order(case["guess"], None, K)               # replaces the first one's half
    assert be.block_sched_peek(first[0], 2) is None
    _sweep(be, case, first, 0, "an order whose table has been replaced")
    _sweep(be, case, third, 1, "third visit order")
    # two contexts, each with its own tables
    be2 = HipBackend(be.device)
    be2.ctx = _lib.Context(be.device.index)                      # (backends of one device share a context otherwise)
    mine = be2.visit_order(case["guess"], case["gdis"], K)
    ids2, dis2 = be2.assign_pruned(case["x"], case["c"], mine, case["cperm"], be2.group_min_dist(case["c"], case["cperm"]), filter=True)
    assert be2.block_sched_last()[0] == 1
    assert np.array_equal(ids2.cpu().numpy(), case["ids_o"]) and np.array_equal(bits(dis2.cpu().numpy()), bits(case["dis_o"]))
    ids2, _ = be2.assign_pruned(case["x"], case["c"], third, case["cperm"], be2.group_min_dist(case["c"], case["cperm"]), filter=True)
    assert be2.block_sched_last()[0] == 0 and np.array_equal(ids2.cpu().numpy(), case["ids_o"])   # the other context's order
    _sweep(be, case, third, 1, "the first context, after the second one's calls")
    be2.synchronize()
    be2.ctx.close()
