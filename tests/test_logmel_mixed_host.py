"""The plan and the per-lane Stockham / Bluestein passes of audio_tokens_amd/csrc/logmel_mixed_core.h executed on the
host (64 lanes one after another) against numpy: the index algebra of every even n_fft from 64 to 4096 without a GPU."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
fp = ctypes.POINTER(ctypes.c_float)
ip = ctypes.POINTER(ctypes.c_int)
RADICES = {2, 3, 4, 5, 7, 8}
# n_fft of both forms: odd M (441, 35, 1125), prime M (47, 1019, 2039), every radix, the largest sizes
SMOOTH = [70, 400, 480, 640, 882, 1000, 1200, 1536, 2000, 2250, 3000, 4000, 4050, 4032]
FALLBACK = [66, 94, 362, 2038, 4078, 4094]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("h") / "liblogmel_mixed_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so),
                    str(ROOT / "tests" / "host_harness" / "logmel_mixed_host.cpp")], check=True)
    return ctypes.CDLL(str(so))


def _plan(harness, n_fft, force=0):
    out = np.zeros(14, np.int32)
    harness.lmx_host_plan(n_fft, force, out.ctypes.data_as(ip))
    return int(out[0]), int(out[1]), [int(r) for r in out[3:3 + out[2]]]


def _smooth(m):
    for p in (2, 3, 5, 7):
        while m % p == 0:
            m //= p
    return m == 1


def test_plan_of_every_even_size(harness):
    n_mixed = 0
    for n_fft in range(64, 4097, 2):
        M = n_fft // 2
        form, P, radix = _plan(harness, n_fft)
        assert 1 <= len(radix) <= 11 and set(radix) <= RADICES, (n_fft, radix)
        assert int(np.prod(radix)) == P, (n_fft, radix)
        if _smooth(M):
            assert form == 1 and P == M, n_fft
            n_mixed += 1
        else:
            assert form == 2 and P >= 2 * M - 1 and P <= 4096 and P & (P - 1) == 0 and P < 4 * M, (n_fft, P)
            assert set(radix) <= {2, 4, 8}
        form, P, radix = _plan(harness, n_fft, force=1)   # the switch: form 2 for everybody
        assert form == 2 and P >= 2 * M - 1 and P <= 4096 and int(np.prod(radix)) == P
    assert n_mixed > 100


def test_fp32_remainder_is_the_integer_remainder(harness):
    assert harness.lmx_host_check_mod() == 0


def _signals(rng, n):
    t = np.arange(n)
    return [rng.standard_normal(n), np.sin(2 * np.pi * 37.3 * t / n), np.zeros(n), np.eye(n)[n // 3], np.ones(n)]


@pytest.mark.parametrize("n_fft,force", [(n, 0) for n in SMOOTH + FALLBACK] + [(n, 1) for n in SMOOTH])
def test_complex_transform_and_power_spectrum(harness, n_fft, force):
    M = n_fft // 2
    rng = np.random.default_rng(n_fft)
    for re, im in zip(_signals(rng, M), reversed(_signals(rng, M))):
        z = np.empty(2 * M, np.float32)
        z[0::2], z[1::2] = re, im
        Z = np.zeros(2 * M, np.float32)
        harness.lmx_host_fft(n_fft, force, z.ctypes.data_as(fp), Z.ctypes.data_as(fp))
        ref = np.fft.fft(z[0::2].astype(np.float64) + 1j * z[1::2])
        assert np.abs((Z[0::2] + 1j * Z[1::2]) - ref).max() <= 3e-6 * max(np.abs(ref).max(), 1e-30) + 1e-30
    win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)).astype(np.float32)
    for f in _signals(rng, n_fft):
        f = (f.astype(np.float32) * win).astype(np.float32)
        P = np.zeros(M + 1, np.float32)
        harness.lmx_host_power(n_fft, force, f.ctypes.data_as(fp), P.ctypes.data_as(fp))
        ref = np.abs(np.fft.rfft(f.astype(np.float64))) ** 2
        assert np.abs(P - ref).max() <= 3e-6 * max(ref.max(), 1e-30) + 1e-30
