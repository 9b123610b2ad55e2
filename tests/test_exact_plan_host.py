"""The decisions of the exact pruned search that need no GPU (audio_tokens_amd/csrc/exact_plan.h, used by
csrc/exact_search.cpp): the route of a call for every combination of its seven inputs, the sizing of the redo, and the
fold of a call's 128 statistics words into the context's totals -- against the rules written out here and numpy."""
import ctypes
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SWEEP, TODO, ROWS, FINISH = range(4)           # exact_plan::DistPass
NOTHING, SHORT, LONG = range(3)                # exact_plan::RedoKind
PLAN_FIELDS = ("image_up_front", "prepass_separate", "prepass_fused", "filter", "stage2", "async_form", "sweep_dist", "dist")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("h") / "libexact_plan_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests" / "host_harness" / "exact_plan_host.cpp")], check=True)
    lib = ctypes.CDLL(str(so))
    lib.exact_plan_host_async_redo_wgs.restype = ctypes.c_int64
    lib.exact_plan_host_async_redo_wgs.argtypes = [ctypes.c_int64]
    lib.exact_plan_host_fold.restype = ctypes.c_int64
    return lib


def _route(mode, filt, prepass_done, dist, filter_fused, filter_sync, force_sync):
    """What the driver did before it had a plan, decision by decision in the order it made them: the one function
    template that held the route, the workspace claims, the ring and the four ways to finish."""
    r = dict.fromkeys(PLAN_FIELDS, False)
    r["dist"] = SWEEP
    r["ring_slot"] = False
    if not filt:
        r["image_up_front"] = True                      # prep_fp32_image() right behind the claims
    fuse = filt and mode == 0 and not prepass_done and filter_fused != 0
    r["prepass_fused"] = fuse
    if not prepass_done and not fuse:
        r["prepass_separate"] = True
    if filt:
        r["filter"] = True                              # WS_FILTER_MISC / WS_FILTER_LIST claimed, at_filter_use_slot
        async_form = mode == 0 and not force_sync and filter_sync != 1
        if async_form:
            r["ring_slot"] = True                       # slot = (head + count) % ring; else the spare
        r["sweep_dist"] = bool(dist) and (fuse or mode != 0)          # the sweep's dist_out
        finish_fused = dist and fuse and async_form
        if dist and fuse and not finish_fused:
            r["dist"] = TODO
        elif dist and mode == 0 and not fuse:
            r["dist"] = ROWS
        if mode != 0:
            return r                                    # guess generators: no stage 2
        r["stage2"] = True
        if async_form:
            r["async_form"] = True
            if finish_fused:
                r["dist"] = FINISH
    return r


@pytest.mark.parametrize("combo", list(itertools.product((0, 1), repeat=7)), ids=lambda c: "".join(map(str, c)))
def test_plan_is_the_route_of_every_combination(harness, combo):
    mode, filt, prepass_done, dist, filter_fused, filter_sync, force_sync = combo
    out = (ctypes.c_int * 8)()
    harness.exact_plan_host_plan(*combo, out)
    got = dict(zip(PLAN_FIELDS, out))
    want = _route(*combo)
    ring_slot = want.pop("ring_slot")
    assert got == {f: int(v) for f, v in want.items()}, combo
    assert bool(got["async_form"]) == ring_slot            # a ring slot is taken exactly by the asynchronous form
    if mode:                                               # a guess-only call: no stage 2, no ring slot
        assert not got["stage2"] and not got["async_form"] and got["dist"] == SWEEP
    if not filt:                                           # without the filter: image up front, nothing of the filter claimed
        assert got["image_up_front"] and not got["filter"] and not got["stage2"] and not got["async_form"]
        assert not got["prepass_fused"] and not got["sweep_dist"] and got["dist"] == SWEEP
    else:
        assert not got["image_up_front"]
    assert (got["dist"] == FINISH) == bool(dist and got["prepass_fused"] and got["async_form"])
    assert not (got["prepass_fused"] and got["prepass_separate"])
    assert got["prepass_fused"] or got["prepass_separate"] or prepass_done
    if not dist:
        assert got["dist"] == SWEEP and not got["sweep_dist"]


def test_plan_reads_the_switches_as_the_driver_did(harness):
    """filter_fused: anything but 0 fuses; filter_sync: only 1 forces the synchronous form."""
    out = (ctypes.c_int * 8)()
    for fused, sync, want_fused, want_async in [(2, 0, 1, 1), (-1, 2, 1, 1), (0, -1, 0, 1), (1, 1, 1, 0)]:
        harness.exact_plan_host_plan(0, 1, 0, 1, fused, sync, 0, out)
        assert (out[2], out[5]) == (want_fused, want_async), (fused, sync)


@pytest.mark.parametrize("n,wgs", [(20, 256), (16383, 256), (16384, 256), (16448, 257), (64 * 65535, 65535),
                                   (64 * 65535 + 64, 65535)])
def test_asynchronous_redo_workgroups(harness, n, wgs):
    assert harness.exact_plan_host_async_redo_wgs(n) == wgs


@pytest.mark.parametrize("listed,n,kind,count", [
    (0, 1000, NOTHING, 0), (1, 1000, SHORT, 1), (62, 1000, SHORT, 62),      # 62 * 16 = 992: the last short one
    (63, 1000, LONG, 64),                                                   # the first long one, padded to 64 rows
    (64, 1000, LONG, 64), (65, 1000, LONG, 65),
    (65536, 1 << 20, SHORT, 65535),                                         # short, workgroups clamped
    (65537, 1 << 20, LONG, 65537)])
def test_synchronous_redo_verdict(harness, listed, n, kind, count):
    out = (ctypes.c_int64 * 2)()
    harness.exact_plan_host_sync_redo(ctypes.c_int64(listed), ctypes.c_int64(n), out)
    assert (out[0], out[1]) == (kind, count)


def _record(rng):
    words = rng.integers(1 << 20, 1 << 31, 128).astype(np.uint32)           # junk everywhere ...
    words[4], words[5] = 777001, 555003                                     # ... but the tile counts
    words[64:128] = 1000 + 3 * np.arange(64)                                # ... and the 64 sub-list counters
    return words


def _fold(harness, ring, words, rows, before):
    totals = np.array(before, np.int64)
    listed = harness.exact_plan_host_fold(ring, ctypes.c_void_p(words.ctypes.data), ctypes.c_int64(rows),
                                          ctypes.c_void_p(totals.ctypes.data))
    return totals.tolist(), listed


@pytest.mark.parametrize("slack,long_list", [(0, False), (-1, True)])
def test_fold_matches_numpy_and_is_one_fold_for_both_callers(harness, slack, long_list):
    rng = np.random.default_rng(11)
    words = _record(rng)
    listed = int(words[64:128].astype(np.int64).sum())
    rows = listed * 16 + slack                              # listed * 16 == rows: still short; one above: long
    assert (listed * 16 > rows) == long_list
    before = [10 ** 12, 5, 1 << 40, 7]
    after = [before[0] + rows, before[1] + listed, before[2] + int(words[4]), before[3] + int(words[5])]
    for force_before in (0, 1):
        ring, none = _fold(harness, 1, words, rows, before + [force_before])
        sync, sync_listed = _fold(harness, 0, words, rows, before + [force_before])
        assert ring[:4] == after and sync[:4] == after      # the same totals through the ring and the synchronous form
        assert none == -1 and sync_listed == listed
        assert ring[4] == (1 if long_list else force_before)    # the ring only ever switches the synchronous form on
        assert sync[4] == (force_before if long_list else 0)    # the synchronous form only ever switches it off
