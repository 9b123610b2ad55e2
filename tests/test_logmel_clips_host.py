"""The clip maps of audio_tokens_amd/csrc/logmel_clips.h on the host (no GPU): which clip an output frame or a block of
16 / 32 frames belongs to, and where that clip ends, for a plan of at_frontend_plan_host with too-short clips at every
position and for the uniform batch -- against numpy's searchsorted and divmod."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
N_FFT, HOP = 512, 128
# frames = 1 + L // 128 for L > 256: a too-short first clip, two consecutive too-short clips, exactly one block of 16 (1920)
# and one block plus a frame (2048), the same for blocks of 32 (3968, 4096), the shortest valid clip, a too-short last clip
LENGTHS = [100, 1000, 200, 256, 1920, 2048, 3968, 4096, 5000, 257, 10000, 300, 50]
CHANNELS = [1, 2, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1]
FIELDS = ("clip", "t", "T", "w", "L", "base")


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("h") / "liblogmel_clips_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests" / "host_harness" / "logmel_clips_host.cpp")], check=True)
    return ctypes.CDLL(str(so))


@pytest.fixture(scope="module")
def planned():
    from audio_tokens_amd.backend import HostHelpers
    plan, _, _, tot = HostHelpers().frontend_plan(CHANNELS, LENGTHS, [22050] * len(LENGTHS), 22050, N_FFT, HOP)
    assert plan["too_short"].tolist() == [1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert plan["n_frames"][[4, 5, 6, 7]].tolist() == [16, 17, 32, 33]
    return np.ascontiguousarray(plan), tot


def _lookups(fn, head, x, fpb):
    x = np.ascontiguousarray(x, np.int64)
    out = np.zeros((len(x), 6), np.int64)
    fn(*head, _p(x), ctypes.c_int64(len(x)), ctypes.c_int(fpb), _p(out))
    return {name: out[:, i] for i, name in enumerate(FIELDS)}


def _ends(fn, head, g):
    g = np.ascontiguousarray(g, np.int64)
    out = np.zeros((len(g), 2), np.int64)
    fn(*head, _p(g), ctypes.c_int64(len(g)), _p(out))
    return out[:, 0], out[:, 1]


@pytest.mark.parametrize("fpb,prefix,total", [(0, "first_frame", "n_frames"), (16, "first_block16", "n_blocks16"),
                                              (32, "first_block32", "n_blocks32")])
def test_plan_lookup_is_searchsorted_over_the_clips_with_frames(harness, planned, fpb, prefix, total):
    plan, tot = planned
    wave = np.zeros(tot["mono_floats"], np.float32)
    valid = np.flatnonzero(plan["n_frames"] > 0)
    x = np.arange(tot[total])
    assert len(x) == (plan["n_frames"].sum() if fpb == 0 else (-(-plan["n_frames"] // fpb)).sum())
    want = valid[np.searchsorted(plan[prefix][valid], x, "right") - 1]
    got = _lookups(harness.lmc_host_plan_lookups, (_p(plan), ctypes.c_int64(len(plan)), _p(wave)), x, fpb)
    assert np.array_equal(got["clip"], want)
    assert np.array_equal(got["t"], (x - plan[prefix][want]) * (fpb or 1))
    assert (got["t"] >= 0).all() and (got["t"] < plan["n_frames"][want]).all()
    assert np.array_equal(got["T"], plan["n_frames"][want])
    assert np.array_equal(got["w"], plan["mono_offset"][want]) and np.array_equal(got["L"], plan["out_length"][want])
    assert np.array_equal(got["base"], plan["first_frame"][want])
    assert set(got["clip"].tolist()) == set(valid.tolist())          # every clip with frames is found, no other


@pytest.mark.parametrize("T,n_clips", [(37, 5), (32, 3), (1, 4), (16, 2)])
def test_uniform_lookup_is_divmod(harness, T, n_clips):
    L, stride = (T - 1) * HOP + 300, (T - 1) * HOP + 308
    wave = np.zeros(n_clips * stride, np.float32)
    head = (_p(wave), ctypes.c_int64(L), ctypes.c_int64(stride), ctypes.c_int(T))
    for fpb in (0, 16, 32):
        per_clip = T if fpb == 0 else -(-T // fpb)
        x = np.arange(per_clip * n_clips)
        clip, r = np.divmod(x, per_clip)
        got = _lookups(harness.lmc_host_uniform_lookups, head, x, fpb)
        assert np.array_equal(got["clip"], clip) and np.array_equal(got["t"], r * (fpb or 1))
        assert (got["T"] == T).all() and (got["L"] == L).all()
        assert np.array_equal(got["w"], clip * stride) and np.array_equal(got["base"], clip * T)


def _walk(ends_of, total):
    """The piece walk of the min-max passes, in frames: [(first, end, clip)] from 0 to total."""
    pieces, g = [], 0
    while g < total:
        end, clip = ends_of([g])
        assert end[0] > g, (g, end[0])
        pieces.append((g, int(end[0]), int(clip[0])))
        g = int(end[0])
    return pieces


def test_piece_ends_tile_the_output(harness, planned):
    plan, tot = planned
    head = (_p(plan), ctypes.c_int64(len(plan)))
    pieces = _walk(lambda g: _ends(harness.lmc_host_plan_ends, head, g), tot["n_frames"])
    valid = np.flatnonzero(plan["n_frames"] > 0)
    assert pieces == [(int(plan["first_frame"][c]), int(plan["first_frame"][c] + plan["n_frames"][c]), int(c)) for c in valid]
    assert pieces[0][0] == 0 and pieces[-1][1] == tot["n_frames"]     # no gap, no overlap: each starts where the last ended
    # from anywhere inside a clip, the same end
    g = np.arange(tot["n_frames"])
    end, clip = _ends(harness.lmc_host_plan_ends, head, g)
    want = valid[np.searchsorted(plan["first_frame"][valid], g, "right") - 1]
    assert np.array_equal(clip, want) and np.array_equal(end, plan["first_frame"][want] + plan["n_frames"][want])
    # uniform
    T, n_clips = 37, 5
    pieces = _walk(lambda g: _ends(harness.lmc_host_uniform_ends, (ctypes.c_int(T),), g), T * n_clips)
    assert pieces == [(c * T, (c + 1) * T, c) for c in range(n_clips)]


def test_only_the_plan_map_carries_flags(harness):
    assert harness.lmc_host_has_flags(1) == 1 and harness.lmc_host_has_flags(0) == 0
