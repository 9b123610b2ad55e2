"""Audio straight to tokens (ops.AudioTokenizer, SpecTokenizer.tokenize_audio) and SpectrogramGenerator's ragged route
under normalize=True.

The reference for tokens is the existing file route -- SpectrogramGenerator.run() then SpecTokenizer.run() on the same
clips -- and for one batch IndexFlatL2.search(normalize_rows(spec.T), 1) per clip.  Every comparison is on bytes or
int64 values: nothing here has a tolerance.
"""
import json
import wave as wave_mod
from math import gcd
from pathlib import Path

import numpy as np
import pytest
import torch

import flac_ref as F
from test_gpu_frontend_ragged import signal

pytestmark = pytest.mark.gpu

K = 64
# (extension, channels, rate, length); "silent": digital silence, which normalize=True turns into 0 / 0
KINDS = [("flac", 1, 22050, 3000), ("flac", 2, 44100, 5001), ("wav", 1, 48000, 4000), ("npy", 1, 22050, 2999),
         ("silent", 1, 22050, 2600), ("wav", 2, 44100, 6000), ("npy", 2, 16000, 2500), ("flac", 1, 48000, 3777),
         ("wav", 1, 22050, 200), ("flac", 1, 44100, 9000), ("npy", 1, 22050, 3000), ("wav", 2, 48000, 2000)]
YTIDS = [f"yt{i:03d}abcde" for i in range(len(KINDS))] + ["yt900broken"]
SPLIT = {"train": YTIDS[:9] + YTIDS[12:], "validation": YTIDS[9:12]}
SILENT, SHORT, BROKEN = YTIDS[4], YTIDS[8], YTIDS[12]


def write_wav(path, x, sr):
    with wave_mod.open(str(path), "wb") as f:
        f.setnchannels(x.shape[0]), f.setsampwidth(2), f.setframerate(sr)
        f.writeframes(np.ascontiguousarray(x.T).astype("<i2").tobytes())


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """.flac (mono and stereo), .wav and .npy files of unequal length, rate and channel count; a silent clip, one too
    short for the reflect padding and a .flac that does not decode."""
    root = tmp_path_factory.mktemp("audio_tokens")
    audio = root / "audio" / "bal_train" / "yt"
    audio.mkdir(parents=True)
    for i, (y, (ext, C, sr, L)) in enumerate(zip(YTIDS, KINDS)):
        x = (signal(C, L, 1100 + i) * 20000).astype(np.int64)
        if ext == "flac":
            (audio / f"{y}.flac").write_bytes(F.encode(x, sr, 16, block_size=1152, assignment="mid_side" if C == 2 else None))
        elif ext == "wav":
            write_wav(audio / f"{y}.wav", x, sr)
        elif ext == "silent":
            write_wav(audio / f"{y}.wav", np.zeros_like(x), sr)
        else:
            np.save(audio / f"{y}.npy", (x / 32768.0).astype(np.float32))
            (audio / f"{y}.sr").write_text(str(sr))
    blob = bytearray(F.encode((signal(1, 4000, 1199) * 20000).astype(np.int64), 22050, 16, block_size=1152))
    blob[len(blob) // 2] ^= 0x08
    (audio / f"{BROKEN}.flac").write_bytes(bytes(blob))
    (root / "split.json").write_text(json.dumps(SPLIT))
    return root


def config(corpus, out, **kw):
    from audio_tokens_amd.audio_tokens_config import AudioTokensConfig
    return AudioTokensConfig(
        split_file=str(corpus / "split.json"), audio_source_path=str(corpus / "audio"),
        dest_spec_path=out / "spectrograms", source_spec_path=out / "spectrograms",
        centroids_path=out / "centroids.npy", dest_tokenized_path=str(out / "tok"),
        vocab_size=K, niter=6, clustering_batch_size=6, tokenizer_batch_size=5, spectrogram_batch_size=5, **kw)


def write_centroids(cfg, d, seed=5):
    c = np.random.default_rng(seed).standard_normal((K, d)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    Path(cfg.centroids_path).parent.mkdir(parents=True, exist_ok=True)
    np.save(cfg.centroids_path, c)
    return c


def files_under(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(Path(root).rglob("*.npy"))}


# ---- SpectrogramGenerator, normalize=True: the ragged route against the per-length route -----------------------------------------

def test_generator_normalize_writes_the_same_files_either_way(be, corpus, tmp_path, monkeypatch):
    from audio_tokens_amd.processors import SpectrogramGenerator
    device_copies, decodes = [0], [0]
    real_cpu, real_decode = torch.Tensor.cpu, be.flac_decode

    def counting_cpu(self, *a, **kw):
        device_copies[0] += self.is_cuda
        return real_cpu(self, *a, **kw)

    def counting_decode(blobs):
        decodes[0] += bool(blobs)      # (a decode reads its clips' status back: one copy that is not the front end's)
        return real_decode(blobs)
    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    monkeypatch.setattr(be, "flac_decode", counting_decode)
    written, calls, copies = {}, {}, {}
    for ragged in (True, False):
        cfg = config(corpus, tmp_path / f"ragged_{ragged}", normalize=True)
        gen = SpectrogramGenerator(cfg)
        assert gen.spec_transformer.backend is be
        gen.ragged = ragged
        before, device_copies[0], decodes[0] = be.frontend_calls, 0, 0
        gen.run()
        calls[ragged], copies[ragged] = be.frontend_calls - before, device_copies[0] - decodes[0]
        written[ragged] = files_under(tmp_path / f"ragged_{ragged}")
    kept = [y for y in YTIDS[:12] if y not in (SILENT, SHORT)]          # (nor the broken one)
    want = {f"spectrograms/{s}/{y}.npy" for s in SPLIT for y in SPLIT[s] if y in kept}
    assert set(written[True]) == want and set(written[False]) == want
    for name in want:
        assert written[True][name] == written[False][name], name
        spec = np.load(tmp_path / "ragged_True" / name)
        assert spec.dtype == np.float32 and spec.min() == 0.0 and spec.max() == 1.0
    # batches of 5 in split order: one call per reduced rate pair among a batch's decoded files, one log-mel call, and
    # two device->host copies (the spectrograms, the flags)
    expect_calls = expect_copies = 0
    for split in SPLIT.values():
        for b in range(0, len(split), 5):
            pairs = {(sr // gcd(sr, 22050), 22050 // gcd(sr, 22050))
                     for y in split[b: b + 5] if y != BROKEN for sr in [KINDS[YTIDS.index(y)][2]]}
            expect_calls += (len(pairs) + 1) if pairs else 0
            expect_copies += 2 if pairs else 0
    assert calls[True] == expect_calls and calls[False] == 0
    assert copies[True] == expect_copies


# ---- tokenize_audio against generator-then-tokenizer through files -----------------------------------------------------------------

@pytest.mark.parametrize("name,kw", [("default", {}), ("normalize", {"normalize": True}), ("conv", {"use_convolution": True}),
                                     ("nfft1024", {"n_fft": 1024, "hop_length": 512})])
def test_tokenize_audio_writes_what_the_file_route_writes(be, corpus, tmp_path, name, kw):
    from audio_tokens_amd.processors import SpecTokenizer, SpectrogramGenerator
    cfg = config(corpus, tmp_path / "files", **kw)
    write_centroids(cfg, cfg.n_mels * (cfg.num_kernels if cfg.use_convolution else 1))
    gen = SpectrogramGenerator(cfg)
    gen.run()
    tok = SpecTokenizer(cfg)          # (one object for both routes: the same convolution module)
    tok.return_token_lists = False
    tok.run()
    want = files_under(Path(cfg.dest_tokenized_path))
    skipped = {SHORT, BROKEN} | ({SILENT} if cfg.normalize else set())
    assert set(want) == {f"{s}/{y}.npy" for s in SPLIT for y in SPLIT[s] if y not in skipped}
    direct = tmp_path / "direct"
    for s in SPLIT:
        tok.setup_output_directory(direct / s)
        found = [p for p in map(gen.find_audio_file, SPLIT[s]) if p]
        got = tok.tokenize_audio(found, direct / s)
        assert sorted(got) == sorted(y for y in SPLIT[s] if y not in skipped)
        for y, t in got.items():
            assert t.dtype == np.int64 and np.array_equal(t, np.load(direct / s / f"{y}.npy"))
        # the histogram behind analyze_tokens(): np.bincount of what was written
        counts = np.bincount(np.concatenate(list(got.values())), minlength=K)
        assert np.array_equal(be.to_host(tok._hist), counts)
        assert tok.token_statistics()["total"] == counts.sum()
    got = files_under(direct)
    assert set(got) == set(want)
    for f in want:
        assert got[f] == want[f], (name, f)


# ---- AudioTokenizer -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [False, True])
def test_encode_equals_search_on_each_clip(be, corpus, normalize):
    from audio_tokens_amd.ops import AudioTokenizer, IndexFlatL2, LogMelSpectrogram, normalize_rows
    c = np.random.default_rng(9).standard_normal((K, 64)).astype(np.float32)
    arrays = [signal(1, 3000, 1200), signal(2, 5000, 1201), np.zeros((1, 2000), np.float32), signal(1, 256, 1203),
              signal(1, 257, 1204), signal(2, 4001, 1205)]
    rates = [22050, 44100, 22050, 22050, 22050, 48000]
    clips = [torch.from_numpy(a) for a in arrays]
    clips[1] = clips[1].to(be.device)
    at = AudioTokenizer(c, normalize=normalize, backend=be)
    before = be.frontend_calls
    tokens = at.encode(clips, rates)
    assert be.frontend_calls - before == 3 + 1
    st = LogMelSpectrogram(backend=be)
    specs = st.batch(clips, rates, normalize=normalize)
    index = IndexFlatL2(64, backend=be)
    index.add(c)
    none = [i for i, t in enumerate(tokens) if t is None]
    assert none == ([2, 3] if normalize else [3])          # too short; and, scaled, the silent clip
    kept = []
    for i, t in enumerate(tokens):
        if t is None:
            continue
        _, ids = index.search(normalize_rows(specs[i].T.contiguous(), be), 1)
        assert t.dtype == torch.int64 and t.device.type == "cpu" and tuple(t.shape) == (specs[i].shape[1],)
        assert torch.equal(t, ids[:, 0].cpu()), i
        kept.append(t)
    assert torch.equal(at.last_tokens.cpu(), torch.cat(kept))
    # an empty batch: nothing out, nothing launched
    before = be.frontend_calls
    assert at.encode([]) == [] and at.encode_files([]) == [] and be.frontend_calls == before


def test_encode_files_skips_what_the_generator_skips(be, corpus):
    from audio_tokens_amd.ops import AudioTokenizer
    c = np.random.default_rng(9).standard_normal((K, 64)).astype(np.float32)
    audio = corpus / "audio" / "bal_train" / "yt"
    names = [f"{YTIDS[0]}.flac", f"{BROKEN}.flac", f"{SILENT}.wav", f"{SHORT}.wav", f"{YTIDS[3]}.npy", f"{YTIDS[5]}.wav"]
    for normalize, none in ((False, [1, 3]), (True, [1, 2, 3])):
        at = AudioTokenizer(c, normalize=normalize, backend=be)
        tokens = at.encode_files([audio / n for n in names])
        assert [i for i, t in enumerate(tokens) if t is None] == none
        # file by file: the same tokens as in the batch
        for i, n in enumerate(names):
            alone = at.encode_files([str(audio / n)])[0]
            assert (alone is None) == (tokens[i] is None) and (alone is None or torch.equal(alone, tokens[i])), n
