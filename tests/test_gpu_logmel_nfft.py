"""at_logmel_f32 / at_logmel_minmax_f32 at every even n_fft that is not a power of two (64 .. 4096), on the MI355X,
against tests/logmel_ref.py (the oracle's recipe in numpy float64) with the project's tolerance on every bin: the
mixed-radix form (M = n_fft/2 with prime factors 2, 3, 5, 7), the Bluestein form (every other M) and, through the
switch logmel_fallback, the Bluestein form at the smooth sizes too."""
import dataclasses
import json

import numpy as np
import pytest
import torch

from logmel_ref import logmel_ref, logmel_tolerance, test_clips, tolerance_ratio

pytestmark = pytest.mark.gpu

# (n_fft, hop, n_mels): every radix of form 1 (M = 200, 240, 320, 441, 500, 768, 1500, 2000, 35) ...
SMOOTH = [(400, 160, 64), (480, 120, 40), (640, 160, 64), (882, 441, 64), (1000, 250, 128), (1536, 384, 64),
          (3000, 750, 64), (4000, 1000, 128), (70, 35, 8)]
# ... and form 2 (M = 33, 47, 181, 1019, 2039, 2047)
FALLBACK = [(66, 16, 8), (94, 47, 20), (362, 90, 40), (2038, 512, 64), (4078, 1024, 64), (4094, 1000, 128)]
SR = 22050


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ref(oracle, clips, n_fft, hop, n_mels, fb=None):
    return np.stack([logmel_ref(oracle, c, SR, n_fft, hop, n_mels, fb=fb) for c in clips])


def _check(got, ref, what):
    assert got.shape == ref.shape, what
    print(what, "worst |dP| / tolerance:", tolerance_ratio(got, ref))
    ok = logmel_tolerance(got, ref)
    assert ok.all(), f"{what}: {(~ok).sum()} of {ok.size} bins outside tolerance"


@pytest.fixture()
def fallback(be):
    """forces form 2 for the smooth sizes for one test"""
    def set_(on):
        be.debug_set("logmel_fallback", int(on))
    yield set_
    be.debug_set("logmel_fallback", 0)


@pytest.mark.parametrize("n_fft,hop,n_mels", SMOOTH + FALLBACK)
def test_logmel_even_nfft(be, oracle, n_fft, hop, n_mels):
    """The body of test_gpu_ops.py::test_logmel_other_nfft at the sizes that are not powers of two."""
    L = 30001
    clips = test_clips(n_fft, hop, L)
    ref = _ref(oracle, clips, n_fft, hop, n_mels)
    got = be.logmel(clips, SR, n_fft, hop, n_mels).cpu().numpy()
    assert got.shape == ref.shape == (4, n_mels, 1 + L // hop)
    _check(got, ref, f"n_fft={n_fft}")
    nsilent = min(3, (L - 4000 - n_fft // 2) // hop)
    assert nsilent >= 1 and (got[3, :, -nsilent:] == -100.0).all()
    fm = be.logmel(clips, SR, n_fft, hop, n_mels, frame_major=True).cpu().numpy()
    assert np.array_equal(bits(fm.reshape(4, -1, n_mels)), bits(got.transpose(0, 2, 1)))
    fmn = be.logmel(clips, SR, n_fft, hop, n_mels, frame_major=True, l2norm=True).cpu().numpy()
    assert np.array_equal(bits(fmn), bits(fm / (np.linalg.norm(fm, axis=1, keepdims=True) + 1e-10)))
    fb = oracle.mel_filterbank(SR, n_fft, n_mels)[:, ::-1].copy()          # a user filterbank: mel axis reversed
    rev = be.logmel(clips, SR, n_fft, hop, n_mels, fb=fb).cpu().numpy()
    _check(rev[:, ::-1], ref, f"n_fft={n_fft} reversed filterbank")
    again = be.logmel(clips, SR, n_fft, hop, n_mels).cpu().numpy()          # and back to the library's own
    assert np.array_equal(bits(again), bits(got))


@pytest.mark.parametrize("n_fft,hop,n_mels", SMOOTH)
def test_forced_fallback_at_the_smooth_sizes(be, oracle, fallback, n_fft, hop, n_mels):
    clips = test_clips(n_fft, hop)
    ref = _ref(oracle, clips, n_fft, hop, n_mels)
    form1 = be.logmel(clips, SR, n_fft, hop, n_mels).cpu().numpy()
    fallback(1)
    assert be.debug_get("logmel_fallback") == 1
    form2 = be.logmel(clips, SR, n_fft, hop, n_mels).cpu().numpy()
    _check(form2, ref, f"n_fft={n_fft} form 2")
    assert (form2[3, :, -1] == -100.0).all()
    fallback(0)
    back = be.logmel(clips, SR, n_fft, hop, n_mels).cpu().numpy()           # the tables follow the switch
    assert np.array_equal(bits(back), bits(form1))


@pytest.mark.parametrize("n_fft,hop,n_mels", [(400, 160, 64), (882, 441, 64), (94, 47, 20), (2038, 512, 64)])
def test_strided_clips_and_clips_shorter_than_two_frames(be, oracle, n_fft, hop, n_mels):
    rng = np.random.default_rng(n_fft)
    big = torch.from_numpy((0.1 * rng.standard_normal((3, 12347))).astype(np.float32)).to(be.device)
    for L in (n_fft // 2 + 1, n_fft // 2 + hop + 3, 9001):
        view = big[:, 5:5 + L]                                       # odd row stride, unaligned rows
        assert view.stride(0) == 12347
        got = be.logmel(view, SR, n_fft, hop, n_mels).cpu().numpy()
        ref = _ref(oracle, view.cpu().numpy(), n_fft, hop, n_mels)
        assert got.shape == (3, n_mels, 1 + L // hop)
        _check(got, ref, f"n_fft={n_fft} L={L}")


@pytest.mark.parametrize("n_fft,hop,n_mels", [(400, 160, 64), (1000, 250, 128), (362, 90, 40), (94, 47, 20)])
def test_nan_sample_marks_the_reference_bins(be, oracle, n_fft, hop, n_mels):
    """A NaN sample makes every mel bin of its frames NaN whose filter has a non-zero weight, as in the reference.  A
    filter with no non-zero weight at all (one of the 20 at n_fft 94) is an empty band to the banded mel stage: its bin
    is the clamped zero, -100 dB, in every frame, where the reference's dense product gives NaN * 0 = NaN.  The
    power-of-two kernels have always done the same; pinned here."""
    clips = test_clips(n_fft, hop, L=20000, n=2)
    clips[0, 7777] = np.nan
    with np.errstate(invalid="ignore"):
        ref = _ref(oracle, clips, n_fft, hop, n_mels)
    got = be.logmel(clips, SR, n_fft, hop, n_mels).cpu().numpy()
    empty = (oracle.mel_filterbank(SR, n_fft, n_mels) != 0).sum(0) == 0
    assert empty.sum() == (1 if n_fft == 94 else 0)
    assert np.isnan(ref[0]).any() and not np.isnan(ref[1]).any()
    assert np.array_equal(np.isnan(got[:, ~empty]), np.isnan(ref[:, ~empty]))
    assert (got[:, empty] == -100.0).all()
    fin = ~np.isnan(ref)
    assert logmel_tolerance(np.where(fin, got, 0.0), np.where(fin, ref, 0.0)).all()


def test_minmax_form_equals_logmel_then_scaling(be):
    from audio_tokens_amd.synth import synth_clips
    wave = synth_clips(9, L=30000, seed=5, device=be.device)
    wave[4, 12345] = float("nan")
    spec = be.logmel(wave, SR, 400, 160, 64)
    want = be.minmax_scale_clips(spec.clone())
    got = be.logmel_minmax(wave, SR, 400, 160, 64)
    ok = [i for i in range(9) if i != 4]
    assert torch.equal(got[ok].view(torch.int32), want[ok].view(torch.int32))
    assert bool(torch.isnan(got[4]).all()) and bool(torch.isnan(want[4]).all())
    assert float(got[0].min()) == 0.0 and float(got[0].max()) == 1.0


def test_generator_with_torchaudios_default_n_fft(oracle, tmp_path):
    """n_fft = 400 / hop_length = 160 through SpectrogramGenerator and the files it writes (modelled on
    test_gpu_pipeline.py::test_generator_with_the_readme_hyperparameters)."""
    from pathlib import Path
    from audio_tokens_amd.audio_tokens_config import AudioTokensConfig
    from audio_tokens_amd.processors import SpectrogramGenerator
    from audio_tokens_amd.synth import synth_clips
    ytids = [f"yt{i:03d}abcde" for i in range(5)]
    wave = synth_clips(len(ytids), L=22050 * 2, seed=4242, device="cpu").numpy()
    src = tmp_path / "audio"
    for y, w in zip(ytids, wave):
        p = src / "bal_train" / y[:2]
        p.mkdir(parents=True, exist_ok=True)
        np.save(p / f"{y}.npy", w)
    (tmp_path / "out").mkdir()
    (tmp_path / "out" / "split.json").write_text(json.dumps({"train": ytids[:3], "validation": ytids[3:]}))
    cfg = AudioTokensConfig(
        split_file=str(tmp_path / "out" / "split.json"), audio_source_path=str(src),
        dest_spec_path=tmp_path / "spectrograms", source_spec_path=tmp_path / "spectrograms",
        centroids_path=tmp_path / "out" / "centroids.npy", dest_tokenized_path=str(tmp_path / "tok"),
        vocab_size=32, niter=6, clustering_batch_size=6, tokenizer_batch_size=5, spectrogram_batch_size=4)
    cfg = dataclasses.replace(cfg, n_fft=400, hop_length=160)
    specs = SpectrogramGenerator(cfg).populate_specs(ytids[:3])
    assert len(specs) == 3
    for sp in specs:
        ref = logmel_ref(oracle, wave[ytids.index(sp["filename"][:-4])], SR, 400, 160, 64)
        assert tuple(sp["spec"].shape) == ref.shape == (64, 1 + 44100 // 160)
        _check(sp["spec"].float().cpu().numpy(), ref, sp["filename"])
    SpectrogramGenerator(cfg).run()
    for s, ys in (("train", ytids[:3]), ("validation", ytids[3:])):
        files = sorted((Path(cfg.dest_spec_path) / s).glob("*.npy"))
        assert [f.stem for f in files] == sorted(ys)
        for f in files:
            spec = np.load(f)
            assert spec.dtype == np.float32
            _check(spec, logmel_ref(oracle, wave[ytids.index(f.stem)], SR, 400, 160, 64), f.name)


def test_device_pipeline_at_n_fft_400(be):
    import warnings
    from audio_tokens_amd.pipeline import DevicePipeline
    from audio_tokens_amd.synth import synth_clips
    wave = synth_clips(10, L=22050 * 3, seed=7, device="cuda")
    pipe = DevicePipeline(n_mels=64, vocab_size=64, niter=5, clustering_batch_size=4, n_fft=400, hop_length=160)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = pipe.run(wave[:8], wave[8:])
    T = res.frames_per_clip
    assert T == 1 + 22050 * 3 // 160
    frames = be.logmel(wave, SR, 400, 160, 64, frame_major=True, l2norm=True)
    ids = be.assign(frames, res.centroids, want_dist=False)
    ids = ids[0] if isinstance(ids, tuple) else ids
    assert torch.equal(res.tokens_train.cpu(), ids[:8 * T].cpu())
    assert torch.equal(res.tokens_val.cpu(), ids[8 * T:].cpu())


@pytest.mark.parametrize("n_fft,msg", [(401, "odd n_fft=401 is not supported"), (513, "odd n_fft=513 is not supported"),
                                       (62, "n_fft=62 out of range .an even size from 64 to 4096"),
                                       (4098, "n_fft=4098 out of range .an even size from 64 to 4096")])
def test_rejected_sizes_say_why(be, n_fft, msg):
    from audio_tokens_amd import _lib
    wave = torch.zeros(2, 30000, device=be.device)
    with pytest.raises(_lib.NativeError, match=msg):
        be.logmel(wave, SR, n_fft, 16, 8)
    with pytest.raises(_lib.NativeError, match=msg):
        be.logmel_minmax(wave, SR, n_fft, 16, 8)


def test_two_streams_share_the_table_slot(be):
    """One size on each of two streams, then alternating sizes on one context: the results do not change."""
    a = torch.from_numpy(test_clips(400, 160, L=40000, n=6)).to(be.device)
    want400 = be.logmel(a, SR, 400, 160, 64)
    want2038 = be.logmel(a, SR, 2038, 512, 64)
    want1024 = be.logmel(a, SR, 1024, 256, 64)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(s1):
            g400 = be.logmel(a, SR, 400, 160, 64)
        with torch.cuda.stream(s2):
            g2038 = be.logmel(a, SR, 2038, 512, 64)
        s1.synchronize()
        s2.synchronize()
        assert torch.equal(g400.view(torch.int32), want400.view(torch.int32))
        assert torch.equal(g2038.view(torch.int32), want2038.view(torch.int32))
    for _ in range(3):
        assert torch.equal(be.logmel(a, SR, 400, 160, 64).view(torch.int32), want400.view(torch.int32))
        assert torch.equal(be.logmel(a, SR, 1024, 256, 64).view(torch.int32), want1024.view(torch.int32))
        assert torch.equal(be.logmel(a, SR, 2038, 512, 64).view(torch.int32), want2038.view(torch.int32))


def test_table_cache_transitions(be, oracle):
    """Twelve calls that walk both table slots through every change of their key -- hop (the input of the quad / plain
    decision), n_mels, sample rate, a caller's filterbank and back, n_fft within the general slot, the form (mixed
    radix, power of two, Bluestein) -- run twice on the session backend: every result equals, bit for bit, the same
    single call on a backend whose context has just been created and holds no tables.  (HipBackend() shares the
    process-wide context of its device, resident tables included, so the cold backend is given a context of its own;
    the calls that name only (n_fft, hop, n_mels) run at 22050 Hz.)"""
    from audio_tokens_amd import _lib
    from audio_tokens_amd.backend import HipBackend
    clips = torch.from_numpy(test_clips(512, 128, L=6000, n=2)).to(be.device)
    own, rev = False, True
    calls = [(22050, 512, 128, 64, own), (22050, 512, 400, 64, own), (22050, 512, 400, 136, own),
             (16000, 512, 400, 136, own), (16000, 512, 400, 136, rev), (16000, 512, 400, 136, own),
             (SR, 400, 160, 64, own), (SR, 400, 160, 64, rev), (SR, 1024, 256, 64, own), (SR, 2038, 512, 64, own),
             (SR, 400, 160, 40, own), (22050, 512, 128, 64, own)]

    def run(backend, sr, n_fft, hop, n_mels, user):
        fb = oracle.mel_filterbank(sr, n_fft, n_mels)[:, ::-1].copy() if user else None
        out = backend.logmel(clips, sr, n_fft, hop, n_mels, fb=fb)
        assert tuple(out.shape) == (2, n_mels, 1 + 6000 // hop)
        return out.view(torch.int32)

    want = {}
    for c in calls:
        if c not in want:                                  # one cold context per distinct call, used once
            cold = HipBackend(be.device)
            cold.ctx = _lib.Context(be.device.index)
            assert cold.ctx.handle.value != be.ctx.handle.value
            try:
                want[c] = run(cold, *c)
                torch.cuda.synchronize()
            finally:
                cold.ctx.close()
    assert len(want) == 10
    for rnd in range(2):
        for i, c in enumerate(calls):
            assert torch.equal(run(be, *c), want[c]), f"round {rnd}, call {i + 1}: {c}"
