"""SpectrogramGenerator -- the reference's stage 1 (processors/spectrogram_generator.py:18-146 of
danavery/audio-tokens) on the MI355X log-mel kernel.

Same constructor, methods, outputs (spectrograms/{train,validation}/<ytid>.npy, float32
[n_mels, T]) and skip-and-continue error behaviour.  Differences in HOW, not WHAT:
  * the clips of one batch -- any length, mono or stereo, any rate -- go through the ragged front end: one mono-mix /
    resampler launch per rate pair present and ONE fused STFT -> mel -> dB launch (the reference launches a dozen
    kernels per clip); the whole batch comes back in one device->host copy before the per-file np.save, the per-clip
    NaN / Inf flags in another (SpectrogramGenerator.ragged);
    with normalize=True the per-clip (spec - min) / (max - min) rides in the same log-mel call;
  * with ragged=False: one resampler call per clip (ops.Resample) and one launch per clip length.
.flac files are decoded on the device (ops.load_flac / load_flac_batch: all of a batch in one call) and stay there
through the mono mix and the resampler.  Other audio is decoded on the CPU: torchaudio.load if torchaudio is
importable, otherwise PCM/float .wav through the standard library and raw float32 .npy waveforms (used by the
synthetic tests).
"""
import json
import logging
import os
import shutil
import wave as _wave
from pathlib import Path

import numpy as np
import torch
from tqdm import tqdm

from ..audio_tokens_config import AudioTokensConfig
from ..ops import LogMelSpectrogram, Resample, load_flac, load_flac_batch
from .dataset_splitter import load_split

try:  # optional: only used for decoding when it exists
    import torchaudio as _torchaudio
except Exception:  # pragma: no cover - not installed in the build image
    _torchaudio = None


_FLAC_UNSUPPORTED = -8   # AT_E_FLAC_UNSUPPORTED (include/audio_tokens_amd.h): a stream another decoder might read


def _load_audio(path: Path):
    """-> (waveform float32 [C, L], sample_rate); on the host, except for .flac, which is decoded on the device.
    RuntimeError("Failed to decode audio.") is the one failure the reference skips silently
    (spectrogram_generator.py:98-103)."""
    suffix = path.suffix.lower()
    if suffix == ".flac":
        try:
            return load_flac(path)
        except RuntimeError as e:
            # a stream the native decoder does not read (Ogg-FLAC, 32-bit samples): torchaudio's, where it exists
            if getattr(e, "unsupported", False) and _torchaudio is not None:
                return _torchaudio.load(path)
            raise
    if suffix == ".npy":
        w = np.load(path)
        w = w[None, :] if w.ndim == 1 else w
        sr_file = path.with_suffix(".sr")
        sr = int(sr_file.read_text()) if sr_file.exists() else 22050
        return torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)), sr
    if _torchaudio is not None:
        return _torchaudio.load(path)
    if suffix == ".wav":
        try:
            with _wave.open(str(path), "rb") as f:
                sr, ch, width, nframes = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
                raw = f.readframes(nframes)
        except (_wave.Error, EOFError) as e:
            raise RuntimeError("Failed to decode audio.") from e
        if width == 2:
            a = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
        elif width == 4:
            a = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
        elif width == 1:
            a = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
        else:
            raise RuntimeError("Failed to decode audio.")
        return torch.from_numpy(a.reshape(-1, ch).T.copy()), sr
    raise RuntimeError("Failed to decode audio.")


def load_waveform(audio_file_path, logger):
    """-> (waveform [C, L], sample_rate), or None for a file that fails to decode (logged and skipped)."""
    try:
        return _load_audio(Path(audio_file_path))
    except RuntimeError as e:
        if str(e) == "Failed to decode audio.":
            logger.info(f"skipping {audio_file_path}: {e}")
            return None
        raise


def decode_batch(paths, backend, logger, load=None):
    """The files of one batch as they decode -> one entry per path, in order: (waveform [C, L], sample_rate), or None
    for a path that is None and for a file that fails to decode (logged and skipped, as the reference does).  The
    batch's .flac files go through one device decode and stay on the device; every other file through `load`
    (default: load_waveform).
    Shared by SpectrogramGenerator and ops.AudioTokenizer.encode_files."""
    paths = [Path(p) if p else None for p in paths]
    flacs = [p for p in paths if p and p.suffix.lower() == ".flac"]
    decoded = dict(zip(flacs, zip(load_flac_batch(flacs, backend=backend), backend.flac_status))) if flacs else {}
    out = []
    for path in paths:
        got = None
        if path in decoded:
            got, status = decoded[path]
            if got is None and status == _FLAC_UNSUPPORTED and _torchaudio is not None:
                got = _torchaudio.load(path)   # (Ogg-FLAC, 32-bit samples: as _load_audio does)
            if got is None:
                logger.info(f"skipping {path}: Failed to decode audio.")
        elif path:
            got = load(path) if load else load_waveform(path, logger)
        out.append(got)
    return out


class SpectrogramGenerator:
    # A/B switch: True = batches go through the ragged front end (one launch per rate pair present, one log-mel launch,
    # two device->host copies, whatever the clip lengths, with or without normalize); False = one resampler call per
    # clip and one log-mel launch per distinct length.  Both settings write the same files.
    ragged = True

    def __init__(self, config):
        self.config = config
        self.logger = logging.getLogger(__name__)
        self.spec_transformer = LogMelSpectrogram(
            sample_rate=self.config.common_sr,
            n_mels=self.config.n_mels,
            n_fft=self.config.n_fft,
            hop_length=self.config.hop_length,
        )
        # AmplitudeToDB is fused into the kernel; kept as an attribute name for drop-in code
        self.amplitude_to_db_transformer = None
        self.device = self.spec_transformer.backend.device

        self.data_split = load_split(config.split_file)

    def run(self):
        for split in ["train", "validation"]:
            self.logger.info(f"Creating {split} spectrograms")
            output_dir = Path(self.config.dest_spec_path) / split
            shutil.rmtree(output_dir, ignore_errors=True)
            output_dir.mkdir(parents=True)

            ytids = self.data_split[split]
            for i in tqdm(
                range(0, len(ytids), self.config.spectrogram_batch_size),
                total=len(ytids) // self.config.spectrogram_batch_size,
                position=0,
            ):
                batch_ytids = ytids[i: i + self.config.spectrogram_batch_size]
                specs = self.populate_specs(batch_ytids)

                for spec in specs:
                    ytid = os.path.splitext(spec["filename"])[0]
                    output_file = output_dir / f"{ytid}.npy"
                    np.save(output_file, spec["spec"].cpu())
            self.logger.info(f"{split.capitalize()} spectrograms saved to: {output_dir}")

    def populate_specs(self, source_files):
        """-> [{"filename": str, "spec": Tensor[n_mels, T]}] in input order, bad clips skipped.
        The tensors are views of per-length batch results that already live on the host side of
        one bulk copy when `.cpu()` is called on them (they share storage per batch)."""
        found = [(i, self.find_audio_file(ytid)) for i, ytid in enumerate(source_files)]
        if self.ragged:
            return self._populate_specs_ragged(found)
        # the batch as it decodes (.flac on the device, where the waveforms stay), then mono and one resampler call per clip
        got = decode_batch([p for _, p in found], self.spec_transformer.backend, self.logger, load=self.load_waveform)
        waves = [self.resample(self.convert_to_mono(g[0]), g[1]) for g in got if g is not None]
        names = [f for f, g in zip(found, got) if g is not None]

        # one launch per distinct clip length
        by_len = {}
        for j, w in enumerate(waves):
            by_len.setdefault(w.shape[-1], []).append(j)
        specs_by_j = {}
        for L, js in by_len.items():
            if L <= self.config.n_fft // 2:
                self.logger.debug(f"clips shorter than the reflect padding skipped: {len(js)}")
                continue
            batch = torch.stack([waves[j].reshape(-1).to(self.device) for j in js])
            if self.config.normalize:
                # the batch's log-mel with the per-clip (spec - min) / (max - min) behind it in one call: the extremes come
                # out of the log-mel kernel itself (the reference: three torch reductions and two passes per clip)
                st = self.spec_transformer
                out = st.backend.logmel_minmax(batch, st.sample_rate, st.n_fft, st.hop_length, st.n_mels, fb=st.fb)
            else:
                out = self.spec_transformer(batch)                   # [B, n_mels, T] on the GPU
            finite = torch.isfinite(out).flatten(1).all(dim=1).cpu()
            out = out.cpu()  # one bulk device->host copy; the per-file .cpu() in run() is then free
            for b, j in enumerate(js):
                if not bool(finite[b]):
                    self.check_for_nan_inf(out[b], f"spectrogram {names[j][0]}")
                    self.logger.debug(f"Bad file: {names[j][1]}")
                    continue
                specs_by_j[j] = out[b]
        specs = []
        for j in sorted(specs_by_j):
            specs.append({"filename": os.path.basename(names[j][1]), "spec": specs_by_j[j]})
        return specs

    def _populate_specs_ragged(self, found):
        """populate_specs through the ragged front end: the clips as they were decoded -- any length, mono or stereo,
        any rate -- in one call, the per-clip min-max scaling of normalize=True included; the spectrograms come back
        in one device->host copy and the per-clip NaN / Inf flags in another."""
        st = self.spec_transformer
        got = decode_batch([p for _, p in found], st.backend, self.logger, load=self.load_waveform)
        raw = [g for g in got if g is not None]
        names = [f for f, g in zip(found, got) if g is not None]
        if not raw:
            return []
        out, T, first, bad = st.backend.frontend_ragged([w for w, _ in raw], [sr for _, sr in raw], self.config.common_sr,
                                                        st.n_fft, st.hop_length, st.n_mels, fb=st.fb,
                                                        minmax=bool(self.config.normalize))
        out, bad = out.cpu(), bad.cpu()
        specs, m = [], st.n_mels
        if (T == 0).any():
            self.logger.debug(f"clips shorter than the reflect padding skipped: {int((T == 0).sum())}")
        for j, (i, path) in enumerate(names):
            if T[j] == 0:
                continue
            spec = out[m * int(first[j]): m * (int(first[j]) + int(T[j]))].view(m, int(T[j]))
            if int(bad[j]):
                self.check_for_nan_inf(spec, f"spectrogram {i}")
                self.logger.debug(f"Bad file: {path}")
                continue
            specs.append({"filename": os.path.basename(path), "spec": spec})
        return specs

    def find_audio_file(self, ytid):
        audio_file_path = None
        for source_set in self.config.audio_source_sets:
            stem = f"{self.config.audio_source_path}/{source_set}/{ytid[:2]}/{ytid}"
            for ext in (".flac", ".wav", ".npy"):  # the reference looks for .flac only
                audio_file_path = Path(stem + ext)
                if audio_file_path.exists():
                    return audio_file_path
        self.logger.debug(f"Audio file not found: {audio_file_path}")
        return None

    def load_waveform(self, audio_file_path):
        """-> (waveform [C, L], sample_rate), or None for a file that fails to decode (logged and skipped)."""
        return load_waveform(audio_file_path, self.logger)

    def preprocess_waveform(self, audio_file_path):
        got = self.load_waveform(audio_file_path)
        if got is None:
            return None
        waveform, sr = got
        waveform = self.convert_to_mono(waveform)
        waveform = self.resample(waveform, sr)
        return waveform

    @staticmethod
    def convert_to_mono(waveform):
        if waveform.shape[0] > 1:  # stereo or surround
            return torch.mean(waveform, dim=0, keepdim=True)
        return waveform

    def resample(self, waveform, sr):
        """torchaudio.transforms.Resample(sr, common_sr)(waveform) on the device kernel; the taps of
        the last rate pair stay resident, so a dataset at one native rate builds them once."""
        if sr != self.config.common_sr:
            waveform = Resample(sr, self.config.common_sr, backend=self.spec_transformer.backend)(waveform)
        return waveform

    def generate_mel_spectrogram(self, audio):
        """audio [1, L] -> [n_mels, T] dB (MelSpectrogram + AmplitudeToDB in one kernel)."""
        return self.spec_transformer(audio).squeeze(0)

    @staticmethod
    def normalize_spectrogram(spec):
        return (spec - torch.min(spec)) / (torch.max(spec) - torch.min(spec))

    def check_for_nan_inf(self, data, name="data"):
        if torch.isnan(data).any():
            self.logger.debug(f"Warning: NaN values found in {name}")
            return True
        if torch.isinf(data).any():
            self.logger.debug(f"Warning: Inf values found in {name}")
            return True
        return False


if __name__ == "__main__":
    SpectrogramGenerator(AudioTokensConfig()).run()
