"""The host schedule of Kmeans.train's pruned path: what it queues on the backend, in which order and in which
iteration -- the groupings, their take-up, the pacing, the late regrouping, the three forms of the accumulation.

The spatial grouping of the centroids only decides how much the exact sweep skips, so no bit-equality test sees when
the host regroups or how far it runs ahead.  This file pins that with a recording stand-in for the pruned path (every
search answers with the oracle's exact one) and a helper "thread" that runs its job at once.  It drives train() through
its public call and knobs only and needs no GPU."""
import collections
from concurrent.futures import Future

import numpy as np
import pytest

from oracle_backend import OracleBackend

D, K, ROWS = 64, 1024, 4096        # ROWS < 96 * K: the member-list order doubles as the visiting order
ROWS_SORTED = 96 * K               # the smallest training set whose visiting order is sorted on its own

Call = collections.namedtuple("Call", "name args")


class _Opaque:
    """A placeholder for a device table the stand-in never interprets."""

    def __init__(self, what):
        self.what = what

    def __repr__(self):
        return f"<{self.what}>"


class _Event:
    def __init__(self, be, index):
        self.be, self.index = be, index

    def synchronize(self):
        self.be.note("event.synchronize", index=self.index)

    def elapsed_time(self, other):
        self.be.note("elapsed_time", start=self.index, end=other.index)
        return self.be.iter_ms


class RecordingBackend(OracleBackend):
    """OracleBackend plus what train() calls when `prune` is on, with HipBackend's signatures.  Every search is
    oracle.assign; orders, groupings and hints are passed around and never read; every call is logged."""

    def __init__(self, iter_ms=1.0):
        super().__init__()
        self.iter_ms = iter_ms     # what every elapsed_time() answers
        self.reset()

    def reset(self):
        self.calls, self.searches, self.uploads, self._events = [], [], [], 0

    def note(self, name, **args):
        self.calls.append(Call(name, args))

    def _search(self, x, c, want_dist):
        ids, dis = self.assign(x, c, want_dist)
        self.searches.append(ids)
        return ids, dis

    # -- searches ---------------------------------------------------------------------------
    def assign_pruned(self, x, c, order, cperm, dmin, want_dist=True, mode=0, filter=None, image_current=False):
        self.note("assign_pruned", order=order, cperm=cperm, dmin=dmin, mode=mode, image_current=image_current)
        return self._search(x, c, want_dist)

    def assign_c2f(self, x, c, cperm, dmin, gnbr=None, want_dist=True, coherent=False):
        self.note("assign_c2f", cperm=cperm, dmin=dmin, gnbr=gnbr, coherent=coherent)
        return self._search(x, c, want_dist)

    # -- groupings --------------------------------------------------------------------------
    def group_rows_kd(self, rows, leaf=32):
        self.note("group_rows_kd", rows=np.array(rows, copy=True))
        return super().group_rows_kd(rows, leaf)

    def group_min_dist(self, c, cperm):
        out = _Opaque("dmin")
        self.note("group_min_dist", cperm=cperm, out=out)
        return out

    def group_means(self, c, cperm):
        out = _Opaque("means")
        self.note("group_means", cperm=cperm, out=out)
        return out

    def group_neighbours(self, means, nnb=4):
        out = _Opaque("gnbr")
        self.note("group_neighbours", means=means, nnb=nnb, out=out)
        return out

    def from_host_async(self, a, dtype=None):
        out = self.from_host(a, dtype)
        self.uploads.append(out)
        self.note("from_host_async", out=out)
        return out

    def remember_grouping(self, rows, cperm):
        self.note("remember_grouping", rows=np.array(rows, copy=True), cperm=cperm)
        super().remember_grouping(rows, cperm)

    # -- orders and sums ----------------------------------------------------------------------
    def visit_order(self, ids, dis, k):
        out = _Opaque("visit_order")
        self.note("visit_order", ids=ids, out=out)
        return out

    def visit_order_beside(self, ids, dis, k, sum_out=None):
        self.note("visit_order_beside", ids=ids, with_sum=sum_out is not None)
        if sum_out is not None:
            self.sum_f64(dis, out=sum_out)
        out = _Opaque("visit_order_beside")

        def join():
            self.note("visit_order_beside.join", out=out)
            return out
        return join

    def sum_beside(self, dis, sum_out):
        self.note("sum_beside")
        self.sum_f64(dis, out=sum_out)
        return lambda: self.note("sum_beside.join")

    def centroid_accum(self, x, ids, k, out=None, want_order=False, defer_join=False):
        order = _Opaque("member_order") if want_order else None
        self.note("centroid_accum", ids=ids, want_order=want_order, defer_join=defer_join, order=order)
        part = super().centroid_accum(x, ids, k, out=out)
        return (part, order) if want_order else part

    def centroid_accum_join(self):
        self.note("centroid_accum_join")

    def lloyd_stats_split(self, hassign, cent, n, nsplit_out, parts, stats_row, objs=None):
        self.note("lloyd_stats_split")
        k, d = cent.shape
        self.lloyd_stats(hassign, parts, k, d, stats_row, objs=objs)
        self.split_clusters_device(hassign, cent, n, nsplit_out)

    # -- pacing -------------------------------------------------------------------------------
    def record_event_timed(self):
        ev = _Event(self, self._events)
        self._events += 1
        self.note("record_event_timed", index=ev.index)
        return ev


class _Inline:
    """The helper thread's executor, run at once: a job submitted in one iteration is done by the next."""

    def __init__(self, be):
        self.be = be

    def submit(self, job):
        self.be.note("submit")
        f = Future()
        f.set_result(job())
        return f


def iterations(calls):
    """The log cut behind every iteration (its event and the waiting that follows it) -> ([iteration], epilogue).
    What precedes the loop is the head of iteration 0."""
    its, cur, closing = [], [], False
    for c in calls:
        if closing and c.name not in ("event.synchronize", "elapsed_time"):
            its.append(cur)
            cur, closing = [], False
        cur.append(c)
        if c.name == "record_event_timed":
            closing = True
    if closing:
        its.append(cur)
        cur = []
    return its, cur


def names(calls):
    return [c.name for c in calls]


def where(its, name):
    """Iterations in which `name` was called."""
    return [i for i, it in enumerate(its) for c in it if c.name == name]


def one(calls, name):
    (c,) = [c for c in calls if c.name == name]
    return c.args


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def x():
    return np.random.default_rng(20).standard_normal((ROWS, D)).astype(np.float32)


@pytest.fixture(scope="module")
def x_sorted():
    return np.random.default_rng(21).standard_normal((ROWS_SORTED, D)).astype(np.float32)


@pytest.fixture()
def train(monkeypatch):
    """train(be, x, niter=, **knobs / arguments of Kmeans.train) -> (km, [iteration], epilogue), quietly."""
    from audio_tokens_amd import ops

    def run(be, x, niter=20, km=None, init_centroids=None, sync=True, **knobs):
        monkeypatch.setattr(ops, "_grouper", lambda: _Inline(be))
        if km is None:
            km = ops.Kmeans(D, K, niter=niter, backend=be)
        for name, value in knobs.items():
            assert hasattr(km, name)
            setattr(km, name, value)
        be.reset()
        km.train(x, init_centroids=init_centroids, sync=sync)
        its, tail = iterations(be.calls)
        assert len(its) == km.niter
        return km, its, tail
    return run


SEARCH_FIRST = ["group_min_dist", "group_means", "group_neighbours", "assign_c2f"]
SEARCH_LATER = ["group_min_dist", "assign_pruned"]
MEMBER_ORDER = ["sum_beside", "centroid_accum", "centroid_accum_join", "sum_beside.join"]
BESIDE = ["visit_order_beside", "centroid_accum", "visit_order_beside.join", "centroid_accum_join"]
PLAIN = ["sum_beside", "centroid_accum", "visit_order", "centroid_accum_join", "sum_beside.join"]
PLAIN_LAST = ["sum_beside", "centroid_accum", "centroid_accum_join", "sum_beside.join"]


def closing(it):
    """How iteration `it` ends: statistics and repair, its event, and the wait for the event three iterations old."""
    out = ["lloyd_stats_split", "record_event_timed"]
    if it >= 3:
        out.append("event.synchronize")
    if it >= 4:
        out.append("elapsed_time")
    return out


def test_cold_start_schedule_and_bits(train, x, oracle, capsys):
    be = RecordingBackend(iter_ms=1.0)
    km, its, tail = train(be, x)
    # one grouping on the calling thread before the loop, then the coarse-to-fine search over it
    assert names(its[0]) == ["group_rows_kd"] + SEARCH_FIRST + MEMBER_ORDER + closing(0)
    first = one(its[0], "group_min_dist")["cperm"]
    assert one(its[0], "group_means")["cperm"] is first
    assert one(its[0], "group_neighbours")["nnb"] == 8
    assert one(its[0], "group_neighbours")["means"] is one(its[0], "group_means")["out"]
    c2f = one(its[0], "assign_c2f")
    assert c2f["cperm"] is first and c2f["dmin"] is one(its[0], "group_min_dist")["out"]
    assert c2f["gnbr"] is one(its[0], "group_neighbours")["out"]
    # every later iteration: the pruned sweep over the grouping in use, on the image group_min_dist just built
    for i in range(1, 20):
        head = {2: ["submit", "group_rows_kd"], 3: ["from_host_async"], 14: ["submit", "group_rows_kd"],
                15: ["from_host_async"]}.get(i, [])
        assert names(its[i]) == head + SEARCH_LATER + MEMBER_ORDER + closing(i), i
        sweep = one(its[i], "assign_pruned")
        assert sweep["image_current"] is True and sweep["mode"] == 0
        assert sweep["dmin"] is one(its[i], "group_min_dist")["out"]
        assert sweep["cperm"] is one(its[i], "group_min_dist")["cperm"]
        # the visiting order is the member-list order of the previous accumulation
        assert sweep["order"] is one(its[i - 1], "centroid_accum")["order"]
    # the regrouping of iteration 2 is taken up in iteration 3, the late one (niter - 6) in iteration 15
    assert where(its, "submit") == [2, 14] and where(its, "from_host_async") == [3, 15]
    used = [one(it, "group_min_dist")["cperm"] for it in its]
    assert all(u is first for u in used[:3])
    assert all(u is be.uploads[0] for u in used[3:15]) and all(u is be.uploads[1] for u in used[15:])
    assert first is not be.uploads[0] and len(be.uploads) == 2
    # the accumulation of every iteration: member lists and their order, the objective beside it
    for it in its:
        acc = one(it, "centroid_accum")
        assert acc["want_order"] is True and acc["defer_join"] is True
    # after train(): nothing more to take up; the grouping of the result is remembered for these very centroids
    assert names(tail) == ["remember_grouping"]
    assert tail[0].args["cperm"] is be.uploads[1] and np.array_equal(bits(tail[0].args["rows"]), bits(km.centroids))
    assert km._last_assign is be.searches[-1] and len(be.searches) == 20
    # the stand-in answers exactly
    r = oracle.kmeans_train(x, K, niter=20)
    assert np.array_equal(bits(km.centroids), bits(r.centroids))
    assert np.array_equal(km._last_assign.numpy(), r.assign)
    assert "WARNING clustering 4096 points to 1024 centroids" in capsys.readouterr().err


@pytest.mark.parametrize("niter,iter_ms,late", [(20, 1.0, 14), (20, 0.5, 11), (20, 0.05, 10), (20, 5.0, 14),
                                                (12, 1.0, 6), (10, 1.0, 5), (9, 1.0, None), (9, 0.05, None)])
def test_late_regrouping(train, x, niter, iter_ms, late):
    """Due at niter - 6, or earlier once (niter - it) * iter_ms <= 4.5 -- iter_ms is known from iteration 5 on --
    and never before niter // 2; none below ten iterations; once per training."""
    be = RecordingBackend(iter_ms=iter_ms)
    km, its, tail = train(be, x, niter=niter)
    assert where(its, "submit") == [2] + ([late] if late is not None else [])
    assert where(its, "from_host_async") == [3] + ([late + 1] if late is not None else [])
    assert "from_host_async" not in names(tail)


def test_pacing_three_iterations_ahead(train, x):
    be = RecordingBackend(iter_ms=1.0)
    km, its, tail = train(be, x, niter=12)
    for i, it in enumerate(its):
        assert [c.args["index"] for c in it if c.name == "record_event_timed"] == [i]
        waited = [c.args["index"] for c in it if c.name == "event.synchronize"]
        assert waited == ([i - 3] if i >= 3 else []), i
        timed = [(c.args["start"], c.args["end"]) for c in it if c.name == "elapsed_time"]
        assert timed == ([(i - 4, i - 3)] if i >= 4 else []), i
        # the wait is the last thing of the iteration: the device has three iterations queued while the host sleeps
        assert names(it)[-len(closing(i)):] == closing(i)


def test_regrouping_of_the_last_iteration_is_taken_up_after_the_loop(train, x):
    be = RecordingBackend()
    km, its, tail = train(be, x, niter=3)
    assert where(its, "submit") == [2] and where(its, "from_host_async") == []
    assert names(tail) == ["from_host_async", "remember_grouping"]
    assert tail[1].args["cperm"] is be.uploads[0]


@pytest.mark.parametrize("start", ["centroids_device", "centroids"])
def test_warm_start_from_own_result_regroups_nothing_at_its_start(train, x, oracle, start):
    be = RecordingBackend(iter_ms=1.0)
    km, _, _ = train(be, x)
    ended_with = be.uploads[-1]
    first = km.centroids.copy()
    km, its, tail = train(be, x[::-1].copy(), km=km, init_centroids=getattr(km, start))
    assert names(its[0]) == SEARCH_FIRST + MEMBER_ORDER + closing(0)
    assert where(its, "submit") == [14] and where(its, "from_host_async") == [15]
    assert where(its, "group_rows_kd") == [14]
    used = [one(it, "group_min_dist")["cperm"] for it in its]
    assert all(u is ended_with for u in used[:15]) and all(u is be.uploads[0] for u in used[15:])
    assert names(tail) == ["remember_grouping"] and tail[0].args["cperm"] is be.uploads[0]
    r = oracle.kmeans_train(x[::-1].copy(), K, niter=20, init_centroids=first)
    assert np.array_equal(bits(km.centroids), bits(r.centroids))


def test_warm_start_from_a_foreign_array_regroups_beside_the_first_iteration(train, x, oracle):
    be = RecordingBackend(iter_ms=1.0)
    km, _, _ = train(be, x)
    ended_with = be.uploads[-1]
    foreign = km.centroids.copy()
    km, its, tail = train(be, x, km=km, init_centroids=foreign)
    # submitted before iteration 0 on top of the cached grouping, done (here) when iteration 0 is queued
    assert names(its[0]) == ["submit", "group_rows_kd", "from_host_async"] + SEARCH_FIRST + MEMBER_ORDER + closing(0)
    assert np.array_equal(bits(one(its[0], "group_rows_kd")["rows"]), bits(foreign))
    assert one(its[0], "group_min_dist")["cperm"] is be.uploads[0] and be.uploads[0] is not ended_with
    assert where(its, "submit") == [0, 14] and where(its, "from_host_async") == [0, 15]
    r = oracle.kmeans_train(x, K, niter=20, init_centroids=foreign)
    assert np.array_equal(bits(km.centroids), bits(r.centroids))


def test_warm_start_at_another_shape_groups_on_the_calling_thread_again(train, x):
    be = RecordingBackend(iter_ms=1.0)
    km, _, _ = train(be, x, niter=3)
    km.k = K + 16
    init = x[:K + 16].copy()
    km, its, tail = train(be, x, km=km, init_centroids=init)
    assert names(its[0]) == ["group_rows_kd"] + SEARCH_FIRST + MEMBER_ORDER + closing(0)
    assert np.array_equal(bits(one(its[0], "group_rows_kd")["rows"]), bits(init))
    assert one(its[0], "group_min_dist")["cperm"].numel() == (K + 16 + 31) // 32 * 32
    # a warm start: no regrouping at iteration 2, and none late at three iterations
    assert where(its, "submit") == [] and names(tail) == ["remember_grouping"]


@pytest.mark.parametrize("order_beside", [True, False])
def test_accumulation_forms_with_a_sorted_visiting_order(train, x_sorted, order_beside):
    """96 rows per cluster and more: the visiting order is sorted by distance, beside both accumulations on a stream
    of its own (with the objective) or, order_beside off, on the main stream behind the short-list accumulation."""
    be = RecordingBackend()
    km, its, tail = train(be, x_sorted, niter=3, order_beside=order_beside)
    form = BESIDE if order_beside else PLAIN
    assert names(its[0]) == ["group_rows_kd"] + SEARCH_FIRST + form + closing(0)
    assert names(its[1]) == SEARCH_LATER + form + closing(1)
    assert names(its[2]) == ["submit", "group_rows_kd"] + SEARCH_LATER + PLAIN_LAST + closing(2)
    for i, it in enumerate(its):
        acc = one(it, "centroid_accum")
        assert acc["want_order"] is False and acc["defer_join"] is True
        assert acc["ids"] is be.searches[i]
        if i < 2:
            made = one(it, "visit_order_beside.join" if order_beside else "visit_order")["out"]
            assert one(its[i + 1], "assign_pruned")["order"] is made
            if order_beside:
                started = one(it, "visit_order_beside")
                assert started["ids"] is be.searches[i] and started["with_sum"] is True   # no separate objective sum
    assert names(tail) == ["from_host_async", "remember_grouping"]
    assert km._last_assign is be.searches[2]
    assert len(km.iteration_stats) == 3 and all(np.isfinite(s["obj"]) and s["obj"] > 0 for s in km.iteration_stats)


def test_after_train_lend_and_remember(train, x):
    be = RecordingBackend()
    km, its, tail = train(be, x, niter=4, sync=False)
    assert names(tail) == []                       # sync=False: no host copy of the centroids to remember it by
    ended_with = be.uploads[-1]
    table = km.centroids * np.float32(0.5)
    be.reset()
    km.lend_grouping(table)
    assert names(be.calls) == ["remember_grouping"]
    assert be.calls[0].args["cperm"] is ended_with and np.array_equal(bits(be.calls[0].args["rows"]), bits(table))
    assert be.recall_grouping(table) is ended_with
    be.reset()
    km.lend_grouping(table[:-1])                   # another shape: not this grouping's table
    assert be.calls == []
    km, its, tail = train(be, x, km=km, init_centroids=km.centroids_device, sync=True)
    assert names(tail) == ["remember_grouping"] and tail[0].args["cperm"] is ended_with
    assert be.recall_grouping(km.centroids) is ended_with


def test_prune_off_takes_the_dense_path(x, monkeypatch):
    from audio_tokens_amd import ops
    be = RecordingBackend()
    monkeypatch.setattr(ops, "_grouper", lambda: _Inline(be))
    km = ops.Kmeans(D, K, niter=3, backend=be)
    km.prune = False
    km.train(x)
    assert [n for n in names(be.calls) if n != "lloyd_stats_split"] == ["centroid_accum"] * 3
    assert all(c.args["want_order"] is True and c.args["defer_join"] is False for c in be.calls if c.name == "centroid_accum")
