"""be.logmel_minmax at n_fft = 512 (at_logmel_minmax_f32): the tuned kernel collects every clip's extremes and the
scaling pass of the min-max family, walking the uniform clip map, applies them.

The reference is the reference's own expression in torch, SpectrogramGenerator.normalize_spectrogram, applied to each
clip of be.logmel's output: two fp32 subtractions and one IEEE division per value, so every comparison is on the bit
patterns.  Neighbouring clips differ in amplitude by 0.9 against 1e-4, so an extreme that leaks across a clip boundary
changes bits.  n_mels = 6 and 30 take the pass's 4-byte form, with all clip boundaries inside one 4096-float chunk of
a wavefront; 64 takes the 16-byte form over more than one chunk.  (The wrapper allocates its own output, so an output
that is not 16-byte aligned cannot be reached from here.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_CLIPS, L, HOP, CHUNK = 5, 3000, 128, 4096


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(be, wave, n_mels, nan_clips=()):
    from audio_tokens_amd.processors import SpectrogramGenerator
    base = be.logmel(wave, n_fft=512, hop=HOP, n_mels=n_mels).cpu()
    got = be.logmel_minmax(wave, n_fft=512, hop=HOP, n_mels=n_mels).cpu().numpy()
    assert got.shape == tuple(base.shape) == (N_CLIPS, n_mels, be.num_frames(L, HOP))
    for i in range(N_CLIPS):
        want = SpectrogramGenerator.normalize_spectrogram(base[i]).numpy()
        if i in nan_clips:
            assert np.isnan(want).all() and np.isnan(got[i]).all(), f"clip {i}: a NaN sample makes the whole clip NaN"
        else:
            assert np.isfinite(want).all() and want.min() == 0.0 and want.max() == 1.0
            diff = bits(got[i]) != bits(want)
            assert not diff.any(), f"clip {i} n_mels={n_mels}: {int(diff.sum())} values differ"


@pytest.mark.parametrize("n_mels", [6, 30, 64])
def test_logmel_minmax_is_normalize_spectrogram_of_each_clip(be, n_mels):
    T = be.num_frames(L, HOP)
    if n_mels % 4:
        assert N_CLIPS * T * n_mels > 2 * T * n_mels and 2 * T * n_mels < CHUNK   # boundaries inside a chunk
    else:
        assert N_CLIPS * T * n_mels > CHUNK
    rng = np.random.default_rng(512 + n_mels)
    t = np.arange(L) / 22050.0
    wave = rng.standard_normal((N_CLIPS, L)) * 0.3 + np.sin(2 * np.pi * 440.0 * (1 + np.arange(N_CLIPS))[:, None] * t)
    wave *= np.where(np.arange(N_CLIPS) % 2 == 0, 0.9, 1e-4)[:, None]
    wave = torch.from_numpy(wave.astype(np.float32))
    check(be, wave, n_mels)
    wave[2, 1500] = float("nan")          # between two clips that must stay exact
    check(be, wave, n_mels, nan_clips=(2,))
