"""The oracle's log-mel recipe restated in numpy float64 for every even n_fft (oracle.logmel itself takes powers of two
only): the fp32 periodic Hann window widened to double, reflect padding, np.fft.rfft, |.|^2, the oracle's filterbank in
double, clamp at 1e-10, 10 log10, rounded to fp32.  tests/test_logmel_ref.py pins it: on powers of two it equals
oracle.logmel bit for bit, and torch's own fp32 pipeline stays inside the project's tolerance against it."""
import numpy as np


def hann_f32(n_fft):
    """torch.hann_window(n_fft, periodic=True) in fp32: computed in double, rounded once"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)).astype(np.float32)


def power_spectrogram(wave, n_fft, hop):
    """[T, n_fft/2 + 1] float64 with center=True, T = 1 + L // hop"""
    wave = np.asarray(wave, np.float32).astype(np.float64)
    L = wave.shape[0]
    assert n_fft % 2 == 0 and L > n_fft // 2
    x = np.pad(wave, n_fft // 2, mode="reflect")
    T = 1 + L // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    frames = x[idx] * hann_f32(n_fft).astype(np.float64)
    return np.abs(np.fft.rfft(frames, axis=1)) ** 2


def logmel_ref(oracle, wave, sample_rate=22050, n_fft=512, hop=128, n_mels=64, fb=None):
    """[n_mels, T] float32"""
    fb = oracle.mel_filterbank(sample_rate, n_fft, n_mels) if fb is None else np.asarray(fb, np.float32)
    mel = power_spectrogram(wave, n_fft, hop) @ fb.astype(np.float64)
    with np.errstate(invalid="ignore"):
        db = 10.0 * np.log10(np.where(mel <= 1e-10, 1e-10, mel))     # (a NaN stays NaN, as torch.clamp leaves it)
    return np.ascontiguousarray(db.T).astype(np.float32)


def logmel_tolerance(got, ref):
    """tests/test_gpu_ops.py::_logmel_tolerance: |dP| <= 2e-5 P + 1e-9 max_frame(P) + 1e-14 in the power domain, per bin"""
    P, Pr = 10.0 ** (got.astype(np.float64) / 10), 10.0 ** (ref.astype(np.float64) / 10)
    pmax = Pr.max(axis=-2, keepdims=True)
    return np.abs(P - Pr) <= 2e-5 * Pr + 1e-9 * pmax + 1e-10 * 1e-4


def tolerance_ratio(got, ref):
    """largest |dP| over what logmel_tolerance allows (<= 1 passes)"""
    P, Pr = 10.0 ** (got.astype(np.float64) / 10), 10.0 ** (ref.astype(np.float64) / 10)
    pmax = Pr.max(axis=-2, keepdims=True)
    return float((np.abs(P - Pr) / (2e-5 * Pr + 1e-9 * pmax + 1e-10 * 1e-4)).max())


def test_clips(n_fft, hop, L=30001, n=4):
    """the clips of test_logmel_other_nfft: noise, a 1234.5 Hz sine, noise, noise silent after 4000 samples"""
    rng = np.random.default_rng(n_fft + hop)
    clips = (0.1 * rng.standard_normal((n, L))).astype(np.float32)
    clips[1] = (0.3 * np.sin(2 * np.pi * 1234.5 * np.arange(L) / 22050)).astype(np.float32)
    if n > 3:
        clips[3, 4000:] = 0.0
    return clips


test_clips.__test__ = False
