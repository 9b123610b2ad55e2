"""The ragged front end (HipBackend.frontend_ragged, ops.LogMelSpectrogram.batch, SpectrogramGenerator.ragged): mono mix,
resampler and log-mel for a batch of clips of unequal length, channel count and sample rate.

The reference for bits is the per-clip route, which is held to the oracle's tolerance elsewhere: torch.mean for stereo,
at_resample_f32, then at_logmel_f32 on each clip alone.  A frame depends only on its own n_fft samples and an output
sample only on its own taps, so every comparison is np.array_equal on the bit patterns.  The padding between clips, in
the input and in the intermediate buffer, is NaN: a read across a clip boundary shows up in the bits.
"""
import json
import wave as wave_mod
from math import gcd
from pathlib import Path

import numpy as np
import pytest
import torch

import flac_ref as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
LAYOUTS = [(False, False), (True, False), (True, True)]   # (frame_major, l2norm)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def signal(C, L, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    x = np.stack([np.sin(t * (0.021 + 0.007 * c) + seed + c) for c in range(C)]) * 0.4
    return (x + 0.1 * rng.standard_normal((C, L))).astype(np.float32)


def nan_packed(be, arrays):
    """The clips as views of ONE device buffer full of NaN, 1 .. 3 floats of padding in front of each (so clips start
    at every alignment) and stereo rows 5 floats apart from their length."""
    total = sum(a.shape[0] * (a.shape[1] + 5) + 3 for a in arrays) + 8
    buf = torch.full((total,), NAN, device=be.device)
    views, pos = [], 0
    for i, a in enumerate(arrays):
        pos += 1 + i % 3
        C, L = a.shape
        v = buf[pos: pos + C * (L + 5)].view(C, L + 5)[:, :L]
        v.copy_(torch.from_numpy(a))
        views.append(v)
        pos += C * (L + 5)
    return views


_ref_cache = {}


def per_clip(be, key, w, sr, common_sr, n_fft, hop, n_mels, frame_major, l2norm, mix_on_host=False):
    """The per-clip route -> (mono row, spectrogram or None when too short), as numpy; computed once per key.
    mix_on_host: torch.mean runs where the clip lies, as SpectrogramGenerator.convert_to_mono does for a clip decoded
    on the host (torch's mean over three or more rows does not round the same way on the host and on the device)."""
    k = (key, sr, common_sr, n_fft, hop, n_mels, frame_major, l2norm)
    if k not in _ref_cache:
        w = torch.from_numpy(w)
        if mix_on_host and w.shape[0] > 1:
            w = torch.mean(w, dim=0, keepdim=True)
        w = w.to(be.device)
        if w.shape[0] > 1:
            w = torch.mean(w, dim=0, keepdim=True)
        if sr != common_sr:
            w = be.resample(w, sr, common_sr)
        mono = w.reshape(-1)
        spec = None
        if mono.numel() > n_fft // 2:
            spec = be.logmel(mono[None], common_sr, n_fft, hop, n_mels, frame_major=frame_major, l2norm=l2norm).cpu().numpy()
        _ref_cache[k] = (mono.cpu().numpy(), spec)
    return _ref_cache[k]


def check_batch(be, tag, arrays, rates, common_sr, n_fft, hop, n_mels, layouts=LAYOUTS):
    views = nan_packed(be, arrays)
    for fm, l2 in layouts:
        out, T, first, bad = be.frontend_ragged(views, rates, common_sr, n_fft, hop, n_mels, frame_major=fm, l2norm=l2,
                                                pad_value=NAN)
        got = out.cpu().numpy().reshape(-1)
        last = be.frontend_last
        mono = last["mono"].cpu().numpy()
        assert got.size == int(T.sum()) * n_mels
        for i, (a, sr) in enumerate(zip(arrays, rates)):
            want_mono, want = per_clip(be, (tag, i), a, sr, common_sr, n_fft, hop, n_mels, fm, l2)
            rec = last["plan"][i]
            assert rec["out_length"] == want_mono.size and rec["mono_offset"] % 4 == 0
            row = mono[rec["mono_offset"]: rec["mono_offset"] + want_mono.size]
            assert np.array_equal(bits(row), bits(want_mono)), f"{tag}: mono row of clip {i} (C={a.shape[0]}, sr={sr})"
            if want is None:
                assert T[i] == 0
                continue
            assert T[i] == be.num_frames(want_mono.size, hop)
            mine = got[n_mels * first[i]: n_mels * (first[i] + T[i])]
            assert np.array_equal(bits(mine), bits(want.reshape(-1))), \
                f"{tag}: clip {i} (L={want_mono.size}, T={T[i]}) frame_major={fm} l2norm={l2}: " \
                f"{int((bits(mine) != bits(want.reshape(-1))).sum())} values differ"
        # the padding between the mono rows is still what it was filled with: nobody wrote across a boundary
        used = np.zeros(mono.size, bool)
        for rec in last["plan"]:
            used[rec["mono_offset"]: rec["mono_offset"] + rec["out_length"]] = True
        assert np.isnan(mono[~used]).all()
        assert not bad.cpu().numpy().any()


def length_pattern(n_fft, hop, block, long_clip):
    """Output lengths with a shortest clip between two long ones: the shortest valid length (every sample reflected)
    and one more; one whole block of frames, one sample more and one frame more; a length that is no multiple of 4;
    a multiple of hop and one more than a multiple of hop; one long clip."""
    half = n_fft // 2
    k = half // hop + 3
    odd = k * hop + hop // 2 + 1
    odd += 1 if odd % 4 == 0 else 0
    return [long_clip, half + 1, block * hop, half + 2, (block - 1) * hop, (block - 1) * hop + 1, odd, (k + 2) * hop,
            (k + 2) * hop + 1]


# ---- 1. lengths, tuned kernel --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hop,block", [(128, 32), (512, 16)])   # the prefetch and the non-prefetch form of the 512 kernel
def test_lengths_tuned_kernel(be, hop, block):
    lengths = length_pattern(512, hop, block, 66150)   # 3 s
    assert lengths[1] == 257 and lengths[3] == 258
    arrays = [signal(1, L, 100 + i) for i, L in enumerate(lengths)]
    check_batch(be, ("len512", hop), arrays, [22050] * len(arrays), 22050, 512, hop, 64)


def test_tuned_kernel_other_widths(be):
    """n_mels outside the fused unit-row range (stand-alone l2norm behind the kernel) and one that is no multiple of 4."""
    lengths = [3000, 257, 2000, 4099]
    arrays = [signal(1, L, 150 + i) for i, L in enumerate(lengths)]
    for n_mels in (6, 30):
        check_batch(be, ("widths", n_mels), arrays, [22050] * 4, 22050, 512, 128, n_mels)


# ---- 2. transform sizes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_fft,hop", [(64, 64), (1024, 512), (400, 160), (1022, 256)])
def test_lengths_other_transform_sizes(be, n_fft, hop):
    lengths = length_pattern(n_fft, hop, 4, 130 * hop + 3)
    arrays = [signal(1, L, 200 + i) for i, L in enumerate(lengths)]
    check_batch(be, ("len", n_fft), arrays, [22050] * len(arrays), 22050, n_fft, hop, 40)


# ---- 3. rates and channels ------------------------------------------------------------------------------------------------

def test_rates_and_channels(be):
    rates = [22050, 44100, 48000, 16000, 44100, 22050, 16000, 48000, 44100, 48000]
    chans = [1, 2, 1, 2, 1, 2, 1, 2, 2, 1]
    lengths = [1000, 5000, 3001, 1777, 4096, 2500, 4999, 1000, 511, 2222]   # 511 at 44100 -> 256: too short
    arrays = [signal(C, L, 300 + i) for i, (C, L) in enumerate(zip(chans, lengths))]
    before = be.frontend_calls
    check_batch(be, "rates", arrays, rates, 22050, 512, 128, 64, layouts=[(False, False)])
    assert be.frontend_calls - before == 4 + 1      # four rate pairs, one log-mel call
    assert be.frontend_last["plan"]["too_short"].tolist() == [0] * 8 + [1, 0]
    modes = {int(g["orig_freq"]): int(g["mode"]) for g in be.frontend_last["groups"]}
    assert modes == {22050: 0, 44100: 2, 48000: 2, 16000: 2}


def test_long_clips_span_several_resampler_tiles(be):
    """A tile is ~4000 output samples at 2:1 and ~1000 at 320:147: clips of several tiles, and of one sample past a tile."""
    plan = be.frontend_plan([1, 1], [100, 100], [44100, 48000], 22050, 512, 128)[2]
    t2, t48 = int(plan[0]["out_per_block"]), int(plan[1]["out_per_block"])
    rates = [44100, 48000, 44100, 48000, 44100]
    lengths = [2 * (2 * t2 + 1), -(-(3 * t48 + 1) * 320 // 147), 2 * t2, 700, 2 * t2 - 1]
    chans = [2, 1, 1, 2, 1]
    arrays = [signal(C, L, 350 + i) for i, (C, L) in enumerate(zip(chans, lengths))]
    check_batch(be, "tiles", arrays, rates, 22050, 512, 128, 64, layouts=[(False, False)])


def test_filter_too_long_for_the_tile(be):
    """2999 -> 3000 Hz: 3013 taps per phase, fewer than four input steps fit the LDS segment, so the one-thread-per-sample
    form runs (as in at_resample_f32)."""
    arrays = [signal(C, L, 380 + i) for i, (C, L) in enumerate([(1, 700), (2, 300), (1, 1)])]
    check_batch(be, "simple", arrays, [2999] * 3, 3000, 64, 32, 8, layouts=[(False, False)])
    assert [int(g["mode"]) for g in be.frontend_last["groups"]] == [1]


def test_more_than_two_channels_and_host_clips(be):
    """Surround is mixed by torch.mean on the caller's side; host tensors, 1-D clips and numpy arrays are accepted."""
    a = [signal(3, 2000, 390), signal(1, 1500, 391), signal(2, 1800, 392), signal(1, 900, 393)]
    clips = [torch.from_numpy(a[0]), torch.from_numpy(a[1][0]), a[2], torch.from_numpy(a[3]).to(be.device)]
    rates = [44100, 22050, 48000, 22050]
    out, T, first, bad = be.frontend_ragged(clips, rates, 22050, 512, 128, 64)
    got = out.cpu().numpy()
    for i in range(4):
        # (the surround clip is a host tensor: mixed on the host, on both routes)
        want = per_clip(be, ("surround", i), a[i], rates[i], 22050, 512, 128, 64, False, False, mix_on_host=i == 0)[1]
        assert np.array_equal(bits(got[64 * first[i]: 64 * (first[i] + T[i])]), bits(want.reshape(-1))), f"clip {i}"


# ---- 4. more clips than 65535 -------------------------------------------------------------------------------------------

def test_seventy_thousand_clips(be):
    n, n_mels = 70_000, 16
    rng = np.random.default_rng(7)
    lengths = rng.choice([33, 100, 200], n)
    offs = np.cumsum(lengths) - lengths
    flat = torch.from_numpy((0.3 * rng.standard_normal(int(lengths.sum()))).astype(np.float32)).to(be.device)
    table = [(int(o), 1, int(L)) for o, L in zip(offs, lengths)]
    out, T, first, bad = be.frontend_ragged((flat, table), 22050, 22050, 64, 64, n_mels)
    assert np.array_equal(T, 1 + lengths // 64) and np.array_equal(first, np.cumsum(T) - T)
    got = out.cpu().numpy()
    assert not bad.cpu().numpy().any()
    for L in (33, 100, 200):
        ids = np.flatnonzero(lengths == L)
        rows = flat[torch.from_numpy(offs[ids][:, None] + np.arange(L)).to(be.device)]          # [n_L, L]
        want = torch.cat([be.logmel(rows[c: c + 65535], 22050, 64, 64, n_mels) for c in range(0, len(ids), 65535)])
        per = n_mels * (1 + L // 64)
        mine = got[(n_mels * first[ids])[:, None] + np.arange(per)]
        assert np.array_equal(bits(mine), bits(want.cpu().numpy().reshape(len(ids), per))), L


# ---- 5. bad clips ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_fft,hop,fm,l2", [(512, 128, False, False), (512, 128, True, True), (400, 160, False, False)])
def test_bad_clips_are_flagged_alone(be, n_fft, hop, fm, l2):
    clean = [signal(1, L, 500 + i) for i, L in enumerate([1500, 1200, 700, 1301, 2000])]
    dirty = [a.copy() for a in clean]
    dirty[1][0, 600] = NAN
    dirty[3][0, 0] = float("inf")
    res = {}
    for name, arrays in (("clean", clean), ("dirty", dirty)):
        out, T, first, bad = be.frontend_ragged(nan_packed(be, arrays), 22050, 22050, n_fft, hop, 64, frame_major=fm,
                                                l2norm=l2, pad_value=NAN)
        res[name] = (out.cpu().numpy().reshape(-1), bad.cpu().numpy())
    assert res["clean"][1].tolist() == [0] * 5
    assert (res["dirty"][1] != 0).tolist() == [False, True, False, True, False]
    for i in (0, 2, 4):
        sl = slice(64 * first[i], 64 * (first[i] + T[i]))
        assert np.isfinite(res["dirty"][0][sl]).all()
        assert np.array_equal(bits(res["dirty"][0][sl]), bits(res["clean"][0][sl])), i
    for i in (1, 3):
        assert not np.isfinite(res["dirty"][0][64 * first[i]: 64 * (first[i] + T[i])]).all()


def test_one_clip_and_empty_batches(be):
    a = signal(2, 3000, 600)
    out, T, first, bad = be.frontend_ragged([torch.from_numpy(a)], [44100], 22050, 512, 128, 64)
    want = per_clip(be, "one", a, 44100, 22050, 512, 128, 64, False, False)[1]
    assert T.tolist() == [be.num_frames(1500, 128)] and first.tolist() == [0] and bad.cpu().tolist() == [0]
    assert np.array_equal(bits(out.cpu().numpy()), bits(want.reshape(-1)))
    before = be.frontend_calls
    out, T, first, bad = be.frontend_ragged([], [], 22050, 512, 128, 64)
    assert out.numel() == 0 and len(T) == 0 and len(first) == 0 and bad.numel() == 0 and be.frontend_calls == before
    # every clip too short: no frames, no flags
    out, T, first, bad = be.frontend_ragged([torch.zeros(1, 256), torch.zeros(2, 10)], 22050, 22050, 512, 128, 64)
    assert out.numel() == 0 and T.tolist() == [0, 0] and bad.cpu().tolist() == [0, 0]


def test_logmel_spectrogram_batch(be):
    from audio_tokens_amd.ops import LogMelSpectrogram
    st = LogMelSpectrogram(sample_rate=22050, n_fft=512, hop_length=128, n_mels=64, backend=be)
    a = [signal(1, 2000, 610), signal(1, 200, 611), signal(2, 4000, 612)]
    specs = st.batch([torch.from_numpy(x) for x in a], [22050, 22050, 44100])
    assert specs[1] is None and st.last_bad.cpu().tolist() == [0, 0, 0]
    for i in (0, 2):
        want = per_clip(be, ("batch", i), a[i], [22050, 22050, 44100][i], 22050, 512, 128, 64, False, False)[1]
        assert tuple(specs[i].shape) == want.shape[1:] and np.array_equal(bits(specs[i].cpu().numpy()), bits(want[0]))
    same = st.batch([torch.from_numpy(a[0])])
    assert np.array_equal(bits(same[0].cpu().numpy()), bits(specs[0].cpu().numpy()))


# ---- 6. the stage class ---------------------------------------------------------------------------------------------------------

def test_generator_writes_the_same_files_either_way(be, tmp_path):
    """A directory of .flac (mono and stereo), .wav and .npy files of mixed lengths and rates, one that fails to decode
    and one that is too short: ragged=True and ragged=False write the same files with the same bytes, and the ragged
    run makes 1 + (rate pairs present) native front-end calls per batch, whatever the lengths."""
    from audio_tokens_amd.audio_tokens_config import AudioTokensConfig
    from audio_tokens_amd.processors import SpectrogramGenerator
    kinds = [("flac", 1, 22050, 3000), ("flac", 2, 44100, 5001), ("wav", 1, 48000, 4000), ("npy", 1, 22050, 2999),
             ("flac", 2, 22050, 3000), ("wav", 2, 44100, 6000), ("npy", 2, 16000, 2500), ("flac", 1, 48000, 3777),
             ("wav", 1, 22050, 200), ("flac", 1, 44100, 9000), ("npy", 1, 22050, 3000), ("wav", 2, 48000, 2000)]
    ytids = [f"yt{i:03d}abcde" for i in range(len(kinds))] + ["yt900broken"]
    audio = tmp_path / "audio" / "bal_train" / "yt"
    audio.mkdir(parents=True)
    for i, (y, (ext, C, sr, L)) in enumerate(zip(ytids, kinds)):
        x = (signal(C, L, 700 + i) * 20000).astype(np.int64)
        if ext == "flac":
            (audio / f"{y}.flac").write_bytes(F.encode(x, sr, 16, block_size=1152, assignment="mid_side" if C == 2 else None))
        elif ext == "wav":
            with wave_mod.open(str(audio / f"{y}.wav"), "wb") as f:
                f.setnchannels(C), f.setsampwidth(2), f.setframerate(sr)
                f.writeframes(np.ascontiguousarray(x.T).astype("<i2").tobytes())
        else:
            np.save(audio / f"{y}.npy", (x / 32768.0).astype(np.float32))
            (audio / f"{y}.sr").write_text(str(sr))
    blob = bytearray(F.encode((signal(1, 4000, 799) * 20000).astype(np.int64), 22050, 16, block_size=1152))
    blob[len(blob) // 2] ^= 0x08
    (audio / "yt900broken.flac").write_bytes(bytes(blob))
    (tmp_path / "split.json").write_text(json.dumps({"train": ytids[:9] + ytids[12:], "validation": ytids[9:12]}))
    written, calls = {}, {}
    for ragged in (True, False):
        root = tmp_path / f"ragged_{ragged}"
        cfg = AudioTokensConfig(
            split_file=str(tmp_path / "split.json"), audio_source_path=str(tmp_path / "audio"),
            dest_spec_path=root / "spectrograms", source_spec_path=root / "spectrograms",
            centroids_path=root / "centroids.npy", dest_tokenized_path=str(root / "tok"),
            vocab_size=32, niter=6, clustering_batch_size=6, tokenizer_batch_size=5, spectrogram_batch_size=5)
        gen = SpectrogramGenerator(cfg)
        gen.ragged = ragged
        before = gen.spec_transformer.backend.frontend_calls
        gen.run()
        calls[ragged] = gen.spec_transformer.backend.frontend_calls - before
        written[ragged] = {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*.npy"))}
    assert sorted(written[True]) == sorted(written[False])
    want = {f"spectrograms/{s}/{y}.npy" for s, ys in (("train", ytids[:8]), ("validation", ytids[9:12])) for y in ys}
    assert set(written[True]) == want          # (not the too-short clip 8, not the broken one)
    for name in written[True]:
        assert written[True][name] == written[False][name], name
    # batches of 5 in split order; a batch costs one call per reduced rate pair among its decoded files and one log-mel call
    expect = 0
    for split in (ytids[:9] + ytids[12:], ytids[9:12]):
        for b in range(0, len(split), 5):
            pairs = {(sr // gcd(sr, 22050), 22050 // gcd(sr, 22050))
                     for y in split[b: b + 5] if y in ytids[:12] for sr in [kinds[ytids.index(y)][2]]}
            expect += (len(pairs) + 1) if pairs else 0
    assert calls[True] == expect and calls[False] == 0
