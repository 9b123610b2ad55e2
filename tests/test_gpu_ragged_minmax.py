"""Per-clip min-max scaling on the ragged front end (at_logmel_ragged_minmax_f32: HipBackend.frontend_ragged(minmax=True)).

The reference is the reference's own expression in torch, SpectrogramGenerator.normalize_spectrogram, applied on the host
to every clip of the UN-normalised frontend_ragged output, which tests/test_gpu_frontend_ragged.py pins: two fp32
subtractions and one IEEE division per value, so every comparison is np.array_equal on the bit patterns.  Where the
reference is NaN (torch.min / max propagate a NaN to the whole clip; a constant clip is 0 / 0) the value must be NaN too;
which NaN is not compared: its sign and payload carry nothing.  Inputs are built as that file builds them -- NaN-packed
views, NaN padding in the intermediate buffer -- and neighbouring clips get very different ranges (amplitude 1e-4 beside
0.9), so extremes that leak across a clip boundary change bits.
"""
import numpy as np
import pytest
import torch

from test_gpu_frontend_ragged import LAYOUTS, NAN, bits, length_pattern, nan_packed, signal

pytestmark = pytest.mark.gpu


def same_bits(mine, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(mine), nan), f"{what}: NaN where the reference has none, or the reverse"
    diff = bits(mine)[~nan] != bits(want)[~nan]
    assert not diff.any(), f"{what}: {int(diff.sum())} values differ"


def check_minmax(be, arrays, rates, common_sr, n_fft, hop, n_mels, layouts=LAYOUTS, bad_clips=()):
    """Every clip of the batch, in every layout, against normalize_spectrogram on the un-normalised output; the flags
    against np.isfinite of the reference.  -> (reference per clip, n_frames)."""
    from audio_tokens_amd.processors import SpectrogramGenerator
    views = nan_packed(be, arrays)
    base, T, first, _ = be.frontend_ragged(views, rates, common_sr, n_fft, hop, n_mels, pad_value=NAN)
    base = base.cpu().numpy()
    want = {}
    for i in range(len(arrays)):
        if T[i]:
            spec = torch.from_numpy(base[n_mels * first[i]: n_mels * (first[i] + T[i])]).view(n_mels, int(T[i]))
            want[i] = SpectrogramGenerator.normalize_spectrogram(spec).numpy()
    expect_bad = [i in want and not np.isfinite(want[i]).all() for i in range(len(arrays))]
    assert [i for i, b in enumerate(expect_bad) if b] == sorted(bad_clips)   # the batch holds what its test says
    for fm, l2 in layouts:
        out, T2, first2, bad = be.frontend_ragged(views, rates, common_sr, n_fft, hop, n_mels, frame_major=fm, l2norm=l2,
                                                  pad_value=NAN, minmax=True)
        assert np.array_equal(T2, T) and np.array_equal(first2, first)
        got = out.cpu().numpy().reshape(-1)
        assert got.size == int(T.sum()) * n_mels
        for i, ref in want.items():
            if fm:
                ref = np.ascontiguousarray(ref.T)
            if l2:
                with np.errstate(invalid="ignore"):
                    ref = ref / (np.linalg.norm(ref, axis=1, keepdims=True) + 1e-10)
            mine = got[n_mels * first[i]: n_mels * (first[i] + T[i])].reshape(ref.shape)
            same_bits(mine, ref, f"clip {i} (T={T[i]}) n_fft={n_fft} hop={hop} n_mels={n_mels} frame_major={fm} l2norm={l2}")
        assert (bad.cpu().numpy() != 0).tolist() == expect_bad, (fm, l2)
    return want, T


def ranged(arrays):
    """Neighbours with very different ranges."""
    return [a * np.float32(1e-4 if i % 2 else 0.9) for i, a in enumerate(arrays)]


def ramp_clip(n_fft, hop, block, n_blocks, seed):
    """n_blocks * block frames: silence at the head of the first block (the clip's minimum, -100 dB, only there), a
    quiet middle, and a loud tail that only frames of the last block see (the clip's maximum)."""
    L = n_blocks * block * hop - hop
    x = signal(1, L, seed)
    x[:, : block * hop // 2] = 0.0
    loud = (n_blocks - 1) * block * hop + n_fft // 2
    x[:, block * hop // 2: loud] *= np.float32(0.01)
    x[:, loud:] *= np.float32(2.0)
    return x


def check_ramp(ref, block, n_blocks):
    """(ref: the scaled clip [n_mels, T]) its zeros lie in the first block of frames only, its ones in the last."""
    T = ref.shape[1]
    assert T == n_blocks * block
    lo, hi = np.flatnonzero((ref == 0).any(0)), np.flatnonzero((ref == 1).any(0))
    assert len(lo) and lo.max() < block and len(hi) and hi.min() >= (n_blocks - 1) * block


# ---- 1. lengths and ranges, tuned kernel (the extremes come out of the log-mel kernel) -----------------------------------------

@pytest.mark.parametrize("hop,block", [(128, 32), (512, 16)])
def test_lengths_and_ranges_tuned_kernel(be, hop, block):
    lengths = length_pattern(512, hop, block, 20000)
    assert lengths[1] == 257 and lengths[2] == block * hop and lengths[4] == (block - 1) * hop   # one block + a frame; one block
    lengths.insert(5, 256)                        # too short (T = 0): shares its prefix with the clip behind it
    lengths.append(20001)                         # (the pattern's short clips lie between long ones)
    clean = ranged([signal(1, L, 900 + i) for i, L in enumerate(lengths)])
    n = len(clean)
    clean.append(ramp_clip(512, hop, block, 3, 950))
    two_sided = signal(1, 9000, 951) * np.float32(0.9)     # dB on both sides of zero, and a run of exact zeros (-100 dB)
    two_sided[:, 3000:6000] = 0.0
    clean.append(two_sided)
    want, T = check_minmax(be, clean, [22050] * len(clean), 22050, 512, hop, 64)
    assert T[5] == 0 and T[1] == be.num_frames(257, hop)
    check_ramp(want[n], block, 3)
    base = be.frontend_ragged([torch.from_numpy(two_sided)], 22050, 22050, 512, hop, 64)[0].cpu().numpy()
    assert (base > 0).any() and (base < 0).any() and (base == -100).any()
    # the same batch with a digital-silence clip and a clip with one NaN sample among them: both all NaN and flagged,
    # nobody else touched (check_minmax compares every clip again)
    silent = np.zeros((1, 3000), np.float32)
    poisoned = signal(1, 2500, 952)
    poisoned[0, 700] = NAN
    dirty = clean[:3] + [silent] + clean[3:8] + [poisoned] + clean[8:]
    want, _ = check_minmax(be, dirty, [22050] * len(dirty), 22050, 512, hop, 64, bad_clips=(3, 9))
    assert np.isnan(want[3]).all() and np.isnan(want[9]).all()


def test_tuned_kernel_other_widths(be):
    """n_mels outside the fused unit-row range and one that is no multiple of 4 (the scaling pass's 4-byte form)."""
    lengths = [3000, 257, 2000, 256, 4099, 9000]
    arrays = ranged([signal(1, L, 960 + i) for i, L in enumerate(lengths)])
    for n_mels in (6, 30, 132):
        check_minmax(be, arrays, [22050] * len(arrays), 22050, 512, 128, n_mels)


# ---- 2. the other transforms (the extremes come from the reduction pass over the output) ----------------------------------------

@pytest.mark.parametrize("n_fft,hop,n_mels", [(1024, 512, 40), (400, 160, 30), (1022, 256, 40)])   # Stockham, mixed radix, Bluestein
def test_other_transform_sizes(be, n_fft, hop, n_mels):
    """The long clip and the ramp span several 4096-float chunks of the reduction and scaling passes (more than one
    workgroup in all), the short ones share a chunk."""
    long_frames = 4 * 4096 // n_mels + 1          # the long clip alone is more than one workgroup's four chunks
    lengths = length_pattern(n_fft, hop, 4, long_frames * hop + 3)
    lengths.insert(5, n_fft // 2)                 # too short
    arrays = ranged([signal(1, L, 970 + i) for i, L in enumerate(lengths)])
    n = len(arrays)
    arrays.append(ramp_clip(n_fft, hop, 110, 3, 990))      # 330 frames: its extremes come from different wavefronts
    silent = np.zeros((1, 3 * n_fft), np.float32)
    arrays.insert(2, silent)
    want, T = check_minmax(be, arrays, [22050] * len(arrays), 22050, n_fft, hop, n_mels, bad_clips=(2,))
    assert int(T.sum()) * n_mels > 4 * 4096
    check_ramp(want[n + 1], 110, 3)


# ---- 3. rates and channels ----------------------------------------------------------------------------------------------------------

def test_rates_and_channels(be):
    rates = [44100, 48000, 22050, 44100, 22050, 48000]
    chans = [2, 1, 1, 2, 1, 1]
    lengths = [5000, 3001, 1000, 511, 2500, 4999]           # 511 at 44100 -> 256: too short
    arrays = ranged([signal(C, L, 1000 + i) for i, (C, L) in enumerate(zip(chans, lengths))])
    before = be.frontend_calls
    _, T = check_minmax(be, arrays, rates, 22050, 512, 128, 64, layouts=[(False, False)])
    assert be.frontend_calls - before == 2 * (3 + 1)        # (the un-normalised call, then this one): three rate pairs, one log-mel call
    assert T[3] == 0


# ---- 4. more clips than 65535 --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_fft,hop,choices", [(512, 128, [257, 300, 384, 400]), (64, 64, [33, 100, 200])])
def test_sixty_six_thousand_clips(be, n_fft, hop, choices):
    n, n_mels = 66_000, 16
    rng = np.random.default_rng(11)
    lengths = rng.choice(choices, n)
    offs = np.cumsum(lengths) - lengths
    amp = np.repeat(np.where(np.arange(n) % 2, 1e-4, 0.9), lengths)
    flat = torch.from_numpy((amp * rng.standard_normal(int(lengths.sum()))).astype(np.float32)).to(be.device)
    table = [(int(o), 1, int(L)) for o, L in zip(offs, lengths)]
    base, T, first, _ = be.frontend_ragged((flat, table), 22050, 22050, n_fft, hop, n_mels)
    out, T2, first2, bad = be.frontend_ragged((flat, table), 22050, 22050, n_fft, hop, n_mels, minmax=True)
    assert np.array_equal(T, 1 + lengths // hop) and np.array_equal(T2, T) and np.array_equal(first2, first)
    assert not bad.cpu().numpy().any()
    base, got = base.cpu(), out.cpu().numpy()
    for L in choices:
        ids = np.flatnonzero(lengths == L)
        per = n_mels * (1 + L // hop)
        at = torch.from_numpy((n_mels * first[ids])[:, None] + np.arange(per))
        x = base[at]                                                                   # [n_L, per], un-normalised
        lo, hi = x.min(dim=1, keepdim=True).values, x.max(dim=1, keepdim=True).values
        want = ((x - lo) / (hi - lo)).numpy()                                          # normalize_spectrogram, row by row
        assert np.array_equal(bits(got[at.numpy()]), bits(want)), L
