"""The block-schedule decisions that need no GPU (audio_tokens_amd/csrc/exact_plan.h: the shape of a filter sweep, the
layout of the schedule workspace, and which block order a sweep takes) and the numpy model of the schedules themselves
(tests/block_schedule_ref.py), checked by hand on a 6-tile example."""
import ctypes
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import block_schedule_ref as bs

ROOT = Path(__file__).resolve().parent.parent
IDENTITY, TABLE0, TABLE1, INSTALLED = range(4)       # exact_plan::SchedPath


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("h") / "libblock_schedule_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests" / "host_harness" / "block_schedule_host.cpp")], check=True)
    lib = ctypes.CDLL(str(so))
    lib.block_schedule_host_shape.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_void_p]
    lib.block_schedule_host_path.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                             ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    lib.block_schedule_host_layout.argtypes = [ctypes.c_int64, ctypes.c_void_p]
    lib.block_schedule_host_limits.argtypes = [ctypes.c_void_p]
    return lib


def _limits(harness):
    out = np.zeros(2, np.int64)
    harness.block_schedule_host_limits(out.ctypes.data)
    return int(out[0]), int(out[1])


def _shape_before(fused, d, n, nbv, wps2):
    """(tiles per wave, waves per SIMD) of the kernel at_filter_sweep launched before the plan function existed.  At
    d = 64 these are its own expressions.  At d = 128 it computed the same NB (unused: 4 without a forced filter_nb) but
    always launched <128, 2, ..., 2> on a grid of 64-row blocks, which the plan function states as (2, 2) outright."""
    one_tile = fused and d == 64 and not wps2 and ((nbv == 1) if nbv else n <= 1 << 19)
    wps3 = (not one_tile) and fused and d == 64 and ((nbv == 2) if nbv else n <= 8 << 20) and not wps2
    nb = 1 if one_tile else 2 if (wps3 or nbv == 2) else 4
    if d == 128:
        return 2, 2
    return nb, 4 if one_tile else 3 if wps3 else 2


def test_sweep_shape_is_the_launch_choice_of_every_combination(harness):
    one, two = _limits(harness)
    assert (one, two) == (1 << 19, 8 << 20)
    out = np.zeros(2, np.int32)
    for fused, d, n, nbv, wps2 in itertools.product((0, 1), (64, 128), (20, one, one + 1, two, two + 1), (0, 1, 2, 4), (0, 1)):
        harness.block_schedule_host_shape(fused, d, n, nbv, wps2, out.ctypes.data)
        assert tuple(out) == _shape_before(fused, d, n, nbv, wps2), (fused, d, n, nbv, wps2)


def _path(harness, tags, block_sched=1, exact=1, order=0x1000, n=4097, tiles=2, blocks=65, installed=0):
    t = np.array(tags, np.int64).reshape(6)
    return harness.block_schedule_host_path(block_sched, exact, order, n, tiles, blocks, t.ctypes.data, installed)


def test_sched_path_uses_a_table_only_under_its_tag(harness):
    none = [0, 0, 0]
    mine, other_n, other_ptr, stale = [0x1000, 4097, 1], [0x1000, 4096, 1], [0x2000, 4097, 1], [0x1000, 4097, 0]
    assert _path(harness, mine + none) == TABLE0
    assert _path(harness, none + mine) == TABLE1
    assert _path(harness, other_ptr + mine) == TABLE1
    assert _path(harness, mine + mine) == TABLE0
    for tags in (none + none, other_n + none, other_ptr + other_n, stale + stale):   # another n, another buffer, dropped
        assert _path(harness, tags) == IDENTITY, tags
    assert _path(harness, mine + none, block_sched=0) == IDENTITY                    # the switch
    assert _path(harness, mine + none, exact=0) == IDENTITY                          # guess generators
    assert _path(harness, mine + none, order=0) == IDENTITY                          # a call without an order
    assert _path(harness, mine + none, tiles=3) == IDENTITY
    # the installed schedule: sweeps of exactly its block count, with or without the switch, never a guess generator
    assert _path(harness, mine + none, installed=65) == INSTALLED
    assert _path(harness, none + none, installed=65, block_sched=0) == INSTALLED
    assert _path(harness, mine + none, installed=64) == TABLE0
    assert _path(harness, none + none, installed=64) == IDENTITY
    assert _path(harness, mine + none, installed=65, exact=0) == IDENTITY


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 129, 4097, 65536 * 32, 65536 * 32 + 1, (1 << 32) - 2])
def test_layout_holds_three_tables_that_do_not_overlap(harness, n):
    out = np.zeros(11, np.int64)
    harness.block_schedule_host_layout(n, out.ctypes.data)
    tiles, blocks, chunks = int(out[0]), out[1:4].tolist(), int(out[4])
    chunk, classes = harness.block_schedule_host_constants(2), harness.block_schedule_host_constants(1)
    assert tiles == -(-n // 32) and blocks == [tiles, -(-tiles // 2), -(-tiles // 4)]
    assert chunks == -(-tiles // chunk) and chunks <= 1 << 16         # a grid dimension
    pieces = [(int(out[5]), tiles), (int(out[6]), 4 * 3 * chunks * classes)] + [(int(out[7 + t]), 4 * blocks[t]) for t in range(3)]
    end = 0
    for off, size in pieces:
        assert off >= end and off % 256 == 0
        end = off + size
    assert int(out[10]) >= end and int(out[10]) % 256 == 0


def test_classes_are_the_top_four_bits(harness):
    assert harness.block_schedule_host_constants(0) == bs.WEIGHT_MAX and harness.block_schedule_host_constants(1) == 1 << bs.CLASS_BITS
    for w in range(256):
        assert harness.block_schedule_host_class(w) == w >> 4 == int(bs.block_classes([w], 1)[0])


def test_model_on_six_tiles_by_hand():
    """k = 10, 8 distance bits, 170 rows = five full tiles and one of 10 rows."""
    k, dbits = 10, 8
    key = lambda cluster, field: (cluster << dbits) | field
    rows = ([key(0, f) for f in np.linspace(0, 0x35, 32).astype(int)]             # tile 0: cluster 0, up to 0x35
            + [key(0, 0x36)] * 20 + [key(1, 0x01)] * 12                           # tile 1: clusters 0 and 1
            + [key(1, f) for f in np.linspace(0x02, 0x12, 32).astype(int)]        # tile 2: cluster 1, up to 0x12
            + [key(1, f) for f in np.linspace(0x13, 0xa0, 32).astype(int)]        # tile 3: cluster 1, up to 0xa0
            + [key(2, f) for f in np.linspace(0x00, 0x3f, 32).astype(int)]        # tile 4: cluster 2, up to 0x3f
            + [key(k, 0)] * 10)                                                   # tile 5: rows without a guess
    keys = np.array(rows, np.int64)
    assert keys.size == 170 and (np.diff(keys) >= 0).all()
    w = bs.tile_weights(keys, k, dbits)
    assert w.tolist() == [0x35, 255, 0x12, 0xa0, 0x3f, 255]
    assert bs.block_classes(w, 1).tolist() == [3, 15, 1, 10, 3, 15]
    assert bs.schedule(w, 1).tolist() == [1, 5, 3, 0, 4, 2]
    assert bs.block_classes(w, 2).tolist() == [15, 10, 15] and bs.schedule(w, 2).tolist() == [0, 2, 1]
    assert bs.block_classes(w, 4).tolist() == [15, 15] and bs.schedule(w, 4).tolist() == [0, 1]
    for tiles in (1, 2, 4):
        assert bs.is_schedule_of(bs.schedule(w, tiles), bs.block_classes(w, tiles))
    assert not bs.is_schedule_of([5, 1, 3, 0, 4, 2], bs.block_classes(w, 1))      # index descends inside class 15
    assert not bs.is_schedule_of([1, 5, 0, 3, 4, 2], bs.block_classes(w, 1))      # class ascends
    assert not bs.is_schedule_of([1, 5, 3, 0, 4, 4], bs.block_classes(w, 1))      # not a permutation
    # fewer distance bits are scaled up, more are scaled down; without distances only the two rules are left
    assert bs.tile_weights(np.full(32, 3, np.int64), k, 2).tolist() == [0xc0]
    assert bs.tile_weights(np.full(32, 0xabc, np.int64), k, 12).tolist() == [0xab]
    assert bs.tile_weights(np.array([0] * 40 + [1] * 24 + [k] * 3, np.int64), k, 0).tolist() == [0, 255, 255]


def test_sorted_keys_are_the_visit_order_models():
    import guess_ref as gr
    rng = np.random.default_rng(4)
    ids = rng.integers(-1, 33, 500)
    dis = (rng.random(500) * 4.5).astype(np.float32)
    for d_ in (dis, None):
        keys, order = bs.sorted_keys(ids, d_, 33)
        order_m, hs_m = gr.visit_order_model(ids, d_, 33)
        assert np.array_equal(order, order_m) and np.array_equal(keys >> 8, hs_m)
