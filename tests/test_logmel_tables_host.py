"""The host-side table builders of audio_tokens_amd/csrc/logmel_tables.h -- what all three log-mel kernels' tables are made
with -- against their definitions restated in numpy: the banded form of a mel filterbank (as it is, and widened to
4-aligned quads of bins for the tuned kernel's 16-byte reads), the periodic Hann window, and the layout of a table slot's
blob.  No GPU needed."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
fp = ctypes.POINTER(ctypes.c_float)
ip = ctypes.POINTER(ctypes.c_int)
lp = ctypes.POINTER(ctypes.c_long)

# (nbin, n_mels) and the n_fft whose filterbank has nbin = n_fft / 2 + 1 bins
SHAPES = [(257, 64, 512), (257, 128, 512), (33, 8, 64), (2048, 128, 4094), (201, 40, 400)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("h") / "liblogmel_tables_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so),
                    str(ROOT / "tests" / "host_harness" / "logmel_tables_host.cpp")], check=True)
    lib = ctypes.CDLL(str(so))
    lib.lmt_host_hann.argtypes = [ctypes.c_int, fp]
    lib.lmt_host_hann.restype = None
    lib.lmt_host_bands.argtypes = [fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ip, ip, ip, fp, ctypes.c_long]
    lib.lmt_host_bands.restype = ctypes.c_long
    lib.lmt_host_layout.argtypes = [ctypes.c_long, ctypes.c_int, lp, lp, lp]
    lib.lmt_host_layout.restype = None
    lib.lmt_host_pack.argtypes = [fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_float, fp,
                                  ctypes.c_long, lp]
    lib.lmt_host_pack.restype = ctypes.c_long
    return lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def filterbanks(oracle, nbin, n_mels, n_fft):
    """the oracle's, the same with the mel axis reversed, a dense one with no zero tap, and one with an all-zero filter
    and a filter whose only tap is the last bin"""
    own = np.ascontiguousarray(oracle.mel_filterbank(22050, n_fft, n_mels), dtype=np.float32)
    assert own.shape == (nbin, n_mels)
    rng = np.random.default_rng(nbin * 1000 + n_mels)
    dense = rng.uniform(0.1, 1.0, (nbin, n_mels)).astype(np.float32)
    edge = own.copy()
    edge[:, 2] = 0.0
    edge[:, n_mels - 1] = 0.0
    edge[nbin - 1, n_mels - 1] = 0.75
    return {"own": own, "reversed": np.ascontiguousarray(own[:, ::-1]), "dense": dense, "edge": edge}


def expected_bands(fb, gran):
    nbin, n_mels = fb.shape
    start, ln, off, wts, pad = [], [], [], [], []
    for m in range(n_mels):
        nz = np.flatnonzero(fb[:, m] != 0)
        s, e = (0, 0) if nz.size == 0 else (nz[0] // gran * gran, (nz[-1] // gran + 1) * gran)
        col = np.zeros(e - s, np.float32)
        col[:min(e, nbin) - s] = fb[s:min(e, nbin), m]
        is_pad = np.ones(e - s, bool)
        if nz.size:
            is_pad[nz[0] - s:nz[-1] - s + 1] = False
        start.append(s)
        ln.append((e - s) // gran)
        off.append(sum(len(w) for w in wts))
        wts.append(col)
        pad.append(is_pad)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
    return np.array(start, np.int32), np.array(ln, np.int32), np.array(off, np.int32), cat(wts, np.float32), cat(pad, bool)


def run_bands(harness, fb, gran):
    nbin, n_mels = fb.shape
    start, ln, off = (np.full(n_mels, -7, np.int32) for _ in range(3))
    wts = np.full((nbin + 3) * n_mels, np.nan, np.float32)
    nw = harness.lmt_host_bands(fb.ctypes.data_as(fp), nbin, n_mels, gran, start.ctypes.data_as(ip), ln.ctypes.data_as(ip),
                                off.ctypes.data_as(ip), wts.ctypes.data_as(fp), wts.size)
    assert 0 <= nw <= wts.size
    return start, ln, off, wts[:nw]


@pytest.mark.parametrize("gran", [1, 4])
@pytest.mark.parametrize("nbin,n_mels,n_fft", SHAPES)
def test_band_tables(harness, oracle, nbin, n_mels, n_fft, gran):
    for name, fb in filterbanks(oracle, nbin, n_mels, n_fft).items():
        start, ln, off, wts = run_bands(harness, fb, gran)
        xs, xl, xo, xw, xpad = expected_bands(fb, gran)
        assert np.array_equal(start, xs) and np.array_equal(ln, xl) and np.array_equal(off, xo), (name, gran)
        assert wts.size == xw.size and np.array_equal(bits(wts), bits(xw)), (name, gran)
        # the dense matrix the kernels' banded dot products stand for is the input, bit for bit
        dense = np.zeros((nbin + 3, n_mels), np.float32)
        for m in range(n_mels):
            n = ln[m] * gran
            assert 0 <= start[m] and start[m] + n <= nbin + 3 and 0 <= off[m] and off[m] + n <= wts.size
            dense[start[m]:start[m] + n, m] = wts[off[m]:off[m] + n]
        assert np.array_equal(bits(dense[:nbin]), bits(fb)), (name, gran)
        assert not bits(dense[nbin:]).any()
        empty = ~(fb != 0).any(axis=0)
        assert (start[empty] == 0).all() and (ln[empty] == 0).all()
        if name == "edge":
            assert empty[2] and not empty[n_mels - 1]
            assert start[n_mels - 1] == (nbin - 1) // gran * gran and ln[n_mels - 1] == 1
        if gran == 4:
            assert (start % 4 == 0).all()
            assert not bits(wts[xpad]).any()                       # every padding weight is +0.0f
            assert (start + 4 * ln <= nbin + 3).all()              # no read reaches past the pad bins behind the last one
        else:
            assert not xpad.any() and (ln[~empty] >= 1).all()
            first = fb[start[~empty], np.flatnonzero(~empty)]
            last = fb[(start + ln - 1)[~empty], np.flatnonzero(~empty)]
            assert (first != 0).all() and (last != 0).all()       # the band as it is: non-zero taps at both ends


@pytest.mark.parametrize("n", [64, 400, 512, 4094])
def test_hann_periodic(harness, n):
    got = np.full(n, np.nan, np.float32)
    harness.lmt_host_hann(n, got.ctypes.data_as(fp))
    want = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)).astype(np.float32)
    assert np.array_equal(bits(got), bits(want))
    assert got[0] == 0.0 and got[n // 2] == 1.0


@pytest.mark.parametrize("n_mels", [1, 6, 8, 20, 64, 129])
def test_blob_layout(harness, n_mels):
    for head in (0, 1536, 198):        # none, the tuned kernel's, the general path's at n_fft 66 (not a multiple of 4)
        ints, wts, nint = ctypes.c_long(-1), ctypes.c_long(-1), ctypes.c_long(-1)
        harness.lmt_host_layout(head, n_mels, ctypes.byref(ints), ctypes.byref(wts), ctypes.byref(nint))
        ints, wts, nint = ints.value, wts.value, nint.value
        assert nint == (3 * n_mels + 3) // 4 * 4 and ints == head and wts == head + nint
        assert (wts - ints) * 4 % 16 == 0
        if head % 4 == 0:
            assert ints * 4 % 16 == 0 and wts * 4 % 16 == 0
        # start | len | off | pad | weights behind the head, as one contiguous run that ends the blob
        nbin = 37
        rng = np.random.default_rng(n_mels)
        fb = (rng.uniform(0.1, 1.0, (nbin, n_mels)) * (rng.random((nbin, n_mels)) < 0.3)).astype(np.float32)
        for gran in (1, 4):
            start, ln, off, w = run_bands(harness, fb, gran)
            blob = np.full(head + nint + (nbin + 3) * n_mels, np.nan, np.float32)
            nw = ctypes.c_long(-1)
            words = harness.lmt_host_pack(fb.ctypes.data_as(fp), nbin, n_mels, gran, head, 7.5, blob.ctypes.data_as(fp),
                                          blob.size, ctypes.byref(nw))
            assert nw.value == w.size and words == head + nint + w.size
            assert (blob[:head] == 7.5).all()
            table = blob[ints:wts].view(np.int32)
            assert np.array_equal(table[:3 * n_mels], np.concatenate([start, ln, off]))
            assert not table[3 * n_mels:].any()
            assert np.array_equal(bits(blob[wts:words]), bits(w))
