"""Pins tests/logmel_ref.py (the yardstick of tests/test_gpu_logmel_nfft.py) without a GPU: it equals oracle.logmel bit
for bit where the oracle is defined, and torch's own fp32 pipeline -- an independent implementation that takes every
size -- is inside the project's tolerance against it at the sizes the GPU tests use."""
import numpy as np
import pytest
import torch

from logmel_ref import hann_f32, logmel_ref, logmel_tolerance, test_clips, tolerance_ratio

SIZES = [(400, 160, 64), (480, 120, 40), (640, 160, 64), (882, 441, 64), (1000, 250, 128), (1536, 384, 64),
         (3000, 750, 64), (4000, 1000, 128), (70, 35, 8), (66, 16, 8), (94, 47, 20), (362, 90, 40), (2038, 512, 64),
         (4078, 1024, 64), (4094, 1000, 128)]


@pytest.mark.parametrize("n_fft", [256, 1024, 4096])
def test_recipe_is_the_oracles_on_powers_of_two(oracle, n_fft):
    hop = n_fft // 4
    for clip in test_clips(n_fft, hop)[[0, 1, 3]]:
        ref = oracle.logmel(clip, n_fft=n_fft, hop=hop, n_mels=64)
        got = logmel_ref(oracle, clip, 22050, n_fft, hop, 64)
        assert got.shape == ref.shape
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("n_fft,hop,n_mels", SIZES)
def test_torch_fp32_pipeline_is_inside_the_tolerance(oracle, n_fft, hop, n_mels):
    fb = torch.from_numpy(oracle.mel_filterbank(22050, n_fft, n_mels))
    # the contract's window (periodic Hann computed in double, rounded to fp32): torch.hann_window computes the cosine in
    # fp32, which is off by 1e-3 of the value at a window's edge and would be measured here instead of the transform
    win = torch.from_numpy(hann_f32(n_fft))
    for clip in test_clips(n_fft, hop):
        ref = logmel_ref(oracle, clip, 22050, n_fft, hop, n_mels)
        st = torch.stft(torch.from_numpy(clip), n_fft, hop, window=win, center=True, pad_mode="reflect",
                        return_complex=True)
        mel = (st.real ** 2 + st.imag ** 2).T @ fb
        got = (10.0 * torch.log10(torch.clamp(mel, min=1e-10))).T.numpy()
        assert got.shape == ref.shape == (n_mels, 1 + clip.shape[0] // hop)
        print(n_fft, "torch fp32 / tolerance:", tolerance_ratio(got, ref))
        assert logmel_tolerance(got, ref).all()
