"""FLAC decoding on the device (at_flac_decode_f32, HipBackend.flac_decode, ops.load_flac, SpectrogramGenerator on
.flac files) against streams made by the test-side encoder (tests/flac_ref.py).

The format is lossless: every comparison is exact -- the decoded tensor equals samples / 2^(bps - 1) bit for bit.
Streams are the smallest at which each mechanism can go wrong (pure-Python bit packing costs microseconds a sample).
"""
import json
import wave as wave_mod

import numpy as np
import pytest
import torch

import flac_ref as F

pytestmark = pytest.mark.gpu


def smooth(C, L, bps, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    x = np.stack([np.sin(t * (0.013 + 0.004 * c) + c) for c in range(C)]) * (1 << (bps - 2))
    return (x + rng.integers(-4, 5, (C, L))).astype(np.int64)


def noise(C, L, bps, seed, scale=1.0):
    """Uncorrelated noise over scale * full range, with both extremes of the range present in every channel."""
    rng = np.random.default_rng(seed)
    hi = max(int((1 << (bps - 1)) * scale), 1)
    x = rng.integers(-hi, hi, (C, L))
    if scale == 1.0 and L >= 4:
        x[:, 1] = -(1 << (bps - 1))
        x[:, 2] = (1 << (bps - 1)) - 1
        x[0::2, 3] = -(1 << (bps - 1))          # ... and opposite extremes in the two channels of a pair
        x[1::2, 3] = (1 << (bps - 1)) - 1
    return x


def expected(x, bps):
    return (np.asarray(x, np.float64) / float(1 << (bps - 1))).astype(np.float32)     # exact for bps <= 24


def check(be, items):
    """items: [(bytes, samples or None, sr, bps)] decoded in ONE call; None = the clip must come back as None."""
    res = be.flac_decode([it[0] for it in items])
    assert len(res) == len(items)
    for i, ((blob, x, sr, bps), r) in enumerate(zip(items, res)):
        if x is None:
            assert r is None and be.flac_status[i] != 0, f"clip {i} should have failed"
            continue
        assert r is not None, f"clip {i}: status {be.flac_status[i]}"
        t, sr_out = r
        assert sr_out == sr and t.dtype == torch.float32 and t.is_cuda and tuple(t.shape) == tuple(np.atleast_2d(x).shape)
        want = expected(np.atleast_2d(x), bps)
        got = t.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            f"clip {i}: {int((got != want).sum())} samples differ, first at {np.argwhere(got != want)[:1].tolist()}"
    return res


def item(x, bps, sr=44100, **kw):
    return (F.encode(x, sr, bps, **kw), x, sr, bps)


# ---- block sizes, sample sizes, channels ---------------------------------------------------------------------------

@pytest.mark.parametrize("bs", [16, 17, 192, 255, 256, 257, 576, 4096, 4608, 65535])
def test_block_sizes_with_a_short_last_block(be, bs):
    L = bs + 100 if bs == 65535 else 2 * bs + 5
    check(be, [item(smooth(1, L, 16, bs), 16, block_size=bs)])


def test_variable_block_sizes(be):
    sizes = [16, 17, 192, 255, 256, 257, 576, 4096, 4608, 7]
    check(be, [item(smooth(2, sum(sizes), 16, 1), 16, block_size=sizes, assignment="left_side")])


@pytest.mark.parametrize("bps,in_header", [(8, True), (12, True), (16, True), (16, False), (20, True), (24, True)])
def test_bits_per_sample(be, bps, in_header):
    check(be, [item(smooth(1, 600, bps, bps), bps, block_size=192, bps_in_header=in_header, rate_in_header=in_header,
                    subframe={"type": "fixed", "order": 3, "method": 1 if bps > 16 else 0})])


@pytest.mark.parametrize("C,assignment", [(1, None), (2, None), (2, "left_side"), (2, "side_right"), (2, "mid_side"),
                                          (3, None), (8, None)])
def test_channels_and_assignments(be, C, assignment):
    check(be, [item(smooth(C, 700, 16, C), 16, sr=22050, block_size=256, assignment=assignment)])


@pytest.mark.parametrize("assignment", ["mid_side", "left_side", "side_right"])
@pytest.mark.parametrize("bps", [8, 16, 24])
def test_decorrelation_on_full_scale_noise(be, assignment, bps):
    """Opposite extremes in the two channels: the side channel needs bps + 1 bits."""
    x = noise(2, 300, bps, bps)
    assert abs(int(x[0, 3]) - int(x[1, 3])) == (1 << bps) - 1
    check(be, [item(x, bps, block_size=192, assignment=assignment, subframe={"type": "fixed", "order": 0, "method": 1})])


# ---- subframe types --------------------------------------------------------------------------------------------------

def test_constant_verbatim_and_fixed_orders(be):
    x = smooth(1, 7 * 64, 16, 2)
    x[0, :64] = -1234
    specs = [{"type": "constant"}, {"type": "verbatim"}] + [{"type": "fixed", "order": o} for o in range(5)]
    check(be, [item(x, 16, block_size=64, subframe=lambda f, ch: specs[f])])


def lpc_spec(order, precision, shift, bps, seed):
    """Random coefficients of the full precision, kept small enough in sum for the residual to fit 32 bits."""
    rng = np.random.default_rng(seed)
    lim = (1 << (precision - 1)) - 1
    room = max(((1 << 30) >> (bps - 1) << shift) // order, 1)          # sum |c| * 2^(bps-1) >> shift stays below 2^30
    c = rng.integers(-min(lim, room), min(lim, room) + 1, order)
    c[0] = -lim - 1 if room > lim else c[0]                            # the most negative coefficient the width holds
    return {"type": "lpc", "order": order, "precision": precision, "shift": shift, "coefs": c, "method": 1}


def test_lpc_orders_precisions_and_shifts(be):
    combos = [(o, p, s) for o in (1, 2, 8, 12, 32) for p in (2, 12, 15) for s in (0, 7, 14)]
    specs = [lpc_spec(o, p, s, 16, i) for i, (o, p, s) in enumerate(combos)]
    x = smooth(1, len(specs) * 48, 16, 3)
    check(be, [item(x, 16, block_size=48, subframe=lambda f, ch: specs[f])])


def test_lpc_sum_beyond_32_bits(be):
    x = noise(1, 256, 24, 4)
    x[0, :40] = (1 << 23) - 1                                          # 32 full-scale samples under 32 large coefficients
    spec = {"type": "lpc", "order": 32, "precision": 15, "shift": 14, "coefs": np.full(32, 16383), "method": 1}
    assert 32 * 16383 * ((1 << 23) - 1) > 1 << 32
    check(be, [item(x, 24, block_size=128, subframe=spec)])


# ---- residual coding ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method,param", [(0, 0), (0, 1), (0, 7), (0, 14), (1, 15), (1, 30)])
def test_rice_parameters(be, method, param):
    bps = 16 if method == 0 else 24
    x = noise(1, 400, bps, param, scale=min(1.0, 2.0 ** (param + 1 - bps)))
    check(be, [item(x, bps, block_size=192, subframe={"type": "fixed", "order": 0, "method": method, "param": param})])


@pytest.mark.parametrize("porder", [0, 1, 7])
def test_partition_orders(be, porder):
    """Order 7 on a 256-sample block leaves partitions of 2 samples: the first one, shortened by the predictor order
    2, is empty.  (The short last block of 64 samples allows order 5 at the most.)"""
    check(be, [item(smooth(2, 512 + 64, 16, porder), 16, block_size=256,
                    subframe=lambda f, ch: {"type": "fixed", "order": 2, "partition_order": porder if f < 2 else min(porder, 5)})])


def test_escaped_partitions(be):
    rng = np.random.default_rng(5)
    x = np.concatenate([np.zeros(64, np.int64), rng.integers(-1, 1, 64), rng.integers(-32768, 32768, 64),
                        rng.integers(-20, 20, 64)])[None, :]
    for width in (None, 17):                                            # smallest widths (0, 1, 16), then bps + 1
        check(be, [item(x, 16, block_size=256, subframe={"type": "fixed", "order": 0, "partition_order": 2,
                                                         "escape": (0, 1, 2), "escape_width": width})])


def test_long_unary_run(be):
    x = np.full((1, 192), -16384, np.int64)
    x[0, 100:] = 16384                                                  # a residual of 2^15 at parameter 0: 65 536 zeros
    check(be, [item(x, 16, block_size=192, subframe={"type": "fixed", "order": 1, "param": 0})])


@pytest.mark.parametrize("wasted", [1, 3])
def test_wasted_bits(be, wasted):
    x = noise(2, 400, 16, wasted, scale=0.1) << wasted
    check(be, [item(x, 16, block_size=192, subframe={"type": "fixed", "order": 1, "wasted": wasted}),
               item(x, 16, block_size=192, assignment="left_side",      # the side channel: bps + 1 - wasted bits
                    subframe={"type": "verbatim", "wasted": wasted})])


# ---- whole batches -------------------------------------------------------------------------------------------------------

def batch_items(n=70, seed=6):
    rng = np.random.default_rng(seed)
    items = []
    for i in range(n):
        C, bs = int(rng.choice([1, 2, 3])), int(rng.choice([16, 64, 192, 256, 576]))
        L = int(rng.integers(bs, 4 * bs + 40))
        L += L % bs == 1                                                # (a last block of one sample has no room for order 2)
        bps = int(rng.choice([8, 16, 24]))
        items.append(item(smooth(C, L, bps, 100 + i), bps, sr=int(rng.choice([22050, 44100])), block_size=bs,
                          assignment="mid_side" if C == 2 and i % 2 else None,
                          subframe={"type": "fixed", "order": min(2, bs), "method": 1 if bps == 24 else 0}))
    items.insert(33, item(np.zeros((2, 0), np.int64), 16))              # a valid stream without frames: [2, 0]
    return items


def test_whole_batch_in_one_call(be):
    items = batch_items()
    frames = sum(len(be.flac_index(it[0])[1]) for it in items)
    assert frames > 128                                                 # more than two waves; clips straddle them
    res = check(be, items)
    assert tuple(res[33][0].shape) == (2, 0)
    assert be.flac_decode([]) == []


def test_two_streams_at_once(be):
    a, b = batch_items(20, 7), batch_items(20, 8)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        ra = be.flac_decode([it[0] for it in a])
    with torch.cuda.stream(s2):
        rb = be.flac_decode([it[0] for it in b])
    torch.cuda.synchronize()
    for items, res in ((a, ra), (b, rb)):
        for (blob, x, sr, bps), r in zip(items, res):
            assert np.array_equal(r[0].cpu().numpy(), expected(x, bps)) and r[1] == sr


# ---- error paths: a status, never a fault ------------------------------------------------------------------------------------

def refresh_crc16(data, frame):
    """The frame's CRC-16 recomputed after an edit, so that only the edited field can give the frame away."""
    a, n = frame["offset"], frame["length"]
    data[a + n - 2: a + n] = F.crc16(bytes(data[a: a + n - 2])).to_bytes(2, "big")


def corrupt_streams():
    out = {}
    frames = []
    x = smooth(1, 600, 16, 9)
    good = F.encode(x, 44100, 16, block_size=192, subframe={"type": "fixed", "order": 2}, frames_out=frames)
    f1 = frames[1]
    d = bytearray(good); d[f1["offset"] + f1["length"] - 6] ^= 0x04; out["residual bit"] = bytes(d)
    d = bytearray(good); d[f1["offset"] + 6 + 1] ^= 0x20; out["warm-up bit"] = bytes(d)     # header 6 bytes, subframe header 1
    d = bytearray(good); d[f1["offset"] + f1["length"] - 1] ^= 0x01; out["crc bit"] = bytes(d)
    out["cut mid-frame"] = good[: frames[-1]["offset"] + frames[-1]["length"] // 2]
    # block size 17, fixed order 0, partition order 0 -> 1: 17 is not divisible by 2
    frames = []
    d = bytearray(F.encode(smooth(1, 17, 16, 10), 44100, 16, block_size=17, subframe={"type": "fixed", "order": 0},
                           frames_out=frames))
    at = frames[0]["offset"] + 7 + 1                                    # header (4 + number + size byte + CRC-8), subframe header
    assert d[at] >> 6 == 0 and (d[at] >> 2) & 15 == 0                   # method 00, partition order 0000
    d[at] |= 1 << 2
    refresh_crc16(d, frames[0])
    out["partition order"] = bytes(d)
    # LPC order 1: precision code behind the 16-bit warm-up sample
    frames = []
    spec = {"type": "lpc", "order": 1, "precision": 5, "shift": 2, "coefs": [3]}
    d = bytearray(F.encode(smooth(1, 192, 16, 11), 44100, 16, block_size=192, subframe=spec, frames_out=frames))
    at = frames[0]["offset"] + 6 + 1 + 2
    assert d[at] >> 4 == 4                                              # precision - 1
    d[at] |= 0xF0
    refresh_crc16(d, frames[0])
    out["lpc precision"] = bytes(d)
    return out


def test_corrupt_clips_fail_alone(be):
    bad = corrupt_streams()
    assert len(bad) == 6
    items = []
    for i, (name, blob) in enumerate(bad.items()):
        items.append(item(smooth(2, 500, 16, 20 + i), 16, block_size=192, assignment="mid_side"))
        items.append((blob, None, 44100, 16))
    items.append(item(smooth(1, 300, 16, 30), 16, block_size=64))
    check(be, items)
    status = dict(zip(bad, be.flac_status[1::2]))
    assert status["crc bit"] == 4 and status["cut mid-frame"] == 3       # CRC-16 mismatch; ran past the frame
    assert status["partition order"] == 2 and status["lpc precision"] == 2    # reserved codes
    assert status["residual bit"] > 0 and status["warm-up bit"] == 4


# ---- the single-file surface and the generator ----------------------------------------------------------------------------------

def test_load_flac(be, tmp_path):
    from audio_tokens_amd import ops
    x = smooth(2, 3000, 16, 12)
    blob = F.encode(x, 22050, 16, block_size=1152, assignment="mid_side")
    (tmp_path / "a.flac").write_bytes(blob)
    for src in (tmp_path / "a.flac", str(tmp_path / "a.flac"), blob):
        w, sr = ops.load_flac(src)
        assert sr == 22050 and w.is_cuda and np.array_equal(w.cpu().numpy(), expected(x, 16))
    bad = bytearray(blob); bad[len(bad) // 2] ^= 0x40
    for src in (bytes(bad), b"not a flac file", tmp_path / "missing.flac"):
        with pytest.raises(RuntimeError, match=r"^Failed to decode audio\.$"):
            ops.load_flac(src)
    res = ops.load_flac_batch([tmp_path / "a.flac", bytes(bad), blob])
    assert res[1] is None and all(np.array_equal(res[i][0].cpu().numpy(), expected(x, 16)) for i in (0, 2))
    assert "load_flac" in ops.__all__ and "load_flac_batch" in ops.__all__


def test_generator_reads_flac_like_wav(be, tmp_path):
    """The same 16-bit waveforms stored as .flac and as .wav give bit-identical spectrogram files; an undecodable
    .flac is skipped and the rest are written."""
    from pathlib import Path
    from audio_tokens_amd.audio_tokens_config import AudioTokensConfig
    from audio_tokens_amd.processors import SpectrogramGenerator
    kinds = [(1, 22050), (2, 22050), (1, 44100), (2, 44100), (1, 22050)]
    ytids = [f"yt{i:03d}abcde" for i in range(len(kinds))] + ["yt900broken"]
    cfgs = {}
    for ext in ("flac", "wav"):
        root = tmp_path / ext
        for i, (y, (C, sr)) in enumerate(zip(ytids, kinds)):
            x = smooth(C, sr // 2 + 37 * i, 16, 40 + i)
            p = root / "audio" / "bal_train" / y[:2]
            p.mkdir(parents=True, exist_ok=True)
            if ext == "flac":
                (p / f"{y}.flac").write_bytes(F.encode(x, sr, 16, block_size=4096, assignment="mid_side" if C == 2 else None))
            else:
                with wave_mod.open(str(p / f"{y}.wav"), "wb") as f:
                    f.setnchannels(C), f.setsampwidth(2), f.setframerate(sr)
                    f.writeframes(np.ascontiguousarray(x.T).astype("<i2").tobytes())
        p = root / "audio" / "bal_train" / "yt"
        if ext == "flac":
            blob = bytearray(F.encode(smooth(1, 9000, 16, 50), 22050, 16, block_size=4096))
            blob[len(blob) // 2] ^= 0x08
            (p / "yt900broken.flac").write_bytes(bytes(blob))
        (root / "out").mkdir()
        (root / "out" / "split.json").write_text(json.dumps({"train": ytids[:4], "validation": ytids[4:]}))
        cfgs[ext] = AudioTokensConfig(
            split_file=str(root / "out" / "split.json"), audio_source_path=str(root / "audio"),
            dest_spec_path=root / "spectrograms", source_spec_path=root / "spectrograms",
            centroids_path=root / "out" / "centroids.npy", dest_tokenized_path=str(root / "tok"),
            vocab_size=32, niter=6, clustering_batch_size=6, tokenizer_batch_size=5, spectrogram_batch_size=3)
        SpectrogramGenerator(cfgs[ext]).run()
    for split, ys in (("train", ytids[:4]), ("validation", ytids[4:5])):
        got = sorted((Path(cfgs["flac"].dest_spec_path) / split).glob("*.npy"))
        assert [f.stem for f in got] == sorted(ys)                       # (the broken one is not among them)
        for f in got:
            a, b = np.load(f), np.load(Path(cfgs["wav"].dest_spec_path) / split / f.name)
            assert a.dtype == np.float32 and a.shape == b.shape and a.shape[0] == 64
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f.name
