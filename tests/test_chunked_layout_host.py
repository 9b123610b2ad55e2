"""The layout of the chunked centroid image that needs no GPU (audio_tokens_amd/csrc/chunked_sweep.h, shared by the
producer in csrc/assign.hip and the sweeps of csrc/knn.hip, ip.hip and rq.hip): the 16-byte slot of a row piece, the
accumulator register -> centroid decode that the strict `<` / `>` tie rules rest on, and the tile size."""
import ctypes
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NA = 4          # accumulators per tile of the three sweeps
NTILES = 3


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("h") / "libchunked_layout_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests" / "host_harness" / "chunked_layout_host.cpp")], check=True)
    lib = ctypes.CDLL(str(so))
    lib.chunked_layout_host_centroid_of.restype = ctypes.c_uint
    lib.chunked_layout_host_centroid_of.argtypes = [ctypes.c_uint, ctypes.c_int]
    lib.chunked_layout_host_tile_floats.restype = ctypes.c_longlong
    return lib


def test_slot_is_a_permutation_of_the_16_slots_of_every_row(harness):
    for r in range(32 * NA):
        slots = sorted(harness.chunked_layout_host_slot(r, q, h) for q in range(8) for h in range(2))
        assert slots == list(range(16)), r
        assert harness.chunked_layout_host_slot(r, 0, 0) == r & 15      # swizzled by the row; 16 rows apart repeat


def test_decode_is_injective_ascending_and_covers_every_centroid(harness):
    ncodes = NTILES * NA * 16
    per_h = []
    for h in range(2):
        ids = [harness.chunked_layout_host_centroid_of(code, h) for code in range(ncodes)]
        assert len(set(ids)) == ncodes                                   # injective
        assert all(b > a for a, b in zip(ids, ids[1:])), h               # strictly ascending in the code
        per_h.append(ids)
    assert set(per_h[0]).isdisjoint(per_h[1])                            # the half-waves hold disjoint centroids
    assert sorted(per_h[0] + per_h[1]) == list(range(NTILES * 32 * NA))  # and together every one of them: [0, 384)


def test_decode_from_the_code_is_base_plus_register_offset(harness):
    for h in range(2):
        for code in range(NTILES * NA * 16):
            assert harness.chunked_layout_host_centroid_of(code, h) == \
                harness.chunked_layout_host_acc_base_plus_offset(code >> 4, code & 15, h)


@pytest.mark.parametrize("d,nchunks", [(4, 1), (64, 1), (68, 2), (128, 2), (640, 10)])
def test_tile_size(harness, d, nchunks):
    assert harness.chunked_layout_host_tile_floats(d, NA) == 128 * 64 * nchunks + 256
    assert harness.chunked_layout_host_buf_floats(NA) == 128 * 64 + 256
