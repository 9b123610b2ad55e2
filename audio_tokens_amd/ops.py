"""MI355X-native stand-ins for the three third-party operators the reference's stage classes call.

    torchaudio.transforms.MelSpectrogram + AmplitudeToDB  ->  LogMelSpectrogram
        (processors/spectrogram_generator.py:28-34,123-126 of danavery/audio-tokens)
    torchaudio.transforms.Resample                        ->  Resample
        (processors/spectrogram_generator.py:117-121)
    faiss.Kmeans                                          ->  Kmeans
        (processors/cluster_creator.py:42-56)
    faiss.IndexFlatL2                                     ->  IndexFlatL2
        (processors/spec_tokenizer.py:123-127, 77)
    faiss.IndexFlatIP                                     ->  IndexFlatIP
        (not used by the reference: the index of Kmeans(spherical=True))
    sklearn.metrics.silhouette_score                      ->  silhouette_score, silhouette_samples
        (processors/cluster_creator.py:115-117)
    sklearn.metrics.average_precision_score (per class)   ->  average_precision, mean_average_precision
        (utils/metrics_calculator.py:8-33; the class itself: audio_tokens_amd.utils.MetricsCalculator)
    sklearn.metrics.f1_score / hamming_loss / roc_auc_score ->  f1_score, hamming_loss, roc_auc, mean_roc_auc,
        (utils/metrics_calculator.py:13-21)                     roc_auc_score, d_prime, classification_metrics
    torchaudio.load (of a .flac file)                     ->  load_flac, load_flac_batch
        (processors/spectrogram_generator.py:99)
    get_spectrogram + get_sequence                        ->  AudioTokenizer
        (tools/manual_tester.py: audio -> tokens against a trained vocabulary)
    faiss.ProductQuantizer, faiss.IndexPQ                 ->  ProductQuantizer, IndexPQ
        (not used by the reference: M code bytes per frame, and the search over them)
    faiss.IndexIVFFlat                                    ->  IndexIVFFlat
        (not used by the reference: the vocabulary as coarse quantiser, exact search of the probed lists)
    faiss.IndexIVFPQ                                      ->  IndexIVFPQ
        (not used by the reference: PQ codes behind the vocabulary's lists, searched without being decoded)
    torchaudio.transforms.MFCC, ComputeDeltas             ->  MFCC, ComputeDeltas
        (not used by the reference: the 13 + delta + delta-delta features of HTK / Kaldi-style tokenisers)

Same constructor arguments, method names, return types and error behaviour as the originals for the
subset the reference uses.  All arithmetic happens in libaudio_tokens_amd.so (HIP, gfx950); this
file is the host-side orchestration: the FAISS training recipe (subsample permutation, random
initialisation, 20 Lloyd iterations, empty-cluster repair) and, when torch.distributed is
initialised and `distributed=True`, the data-parallel variant in which every rank owns a block of
rows and the per-cluster partial sums/counts are exchanged once per iteration.
"""
from __future__ import annotations

import collections
import math
import os
import statistics
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

from .backend import default_backend

__all__ = ["LogMelSpectrogram", "Resample", "Kmeans", "IndexFlatL2", "IndexFlatIP", "normalize_rows", "silhouette_samples",
           "silhouette_score", "average_precision", "mean_average_precision", "roc_auc", "mean_roc_auc",
           "roc_auc_score", "d_prime", "f1_score", "hamming_loss", "classification_metrics", "load_flac",
           "load_flac_batch", "AudioTokenizer", "ProductQuantizer", "ResidualQuantizer", "MFCC", "ComputeDeltas",
           "IndexPQ", "IndexIVFFlat", "IndexIVFPQ"]


def _is_host(x) -> bool:
    return isinstance(x, np.ndarray) or (isinstance(x, torch.Tensor) and x.device.type == "cpu")


def normalize_rows(x, backend=None):
    """x / (||x||_2 + 1e-10) row-wise, bit-identical to the reference's numpy expression
    (cluster_creator.py:64-66).  numpy in -> numpy out; device tensor in -> device tensor out."""
    be = backend or default_backend()
    host = _is_host(x)
    y = be.l2norm_rows(x)
    return be.to_host(y) if host else y


class FlacDecodeError(RuntimeError):
    """The reference's RuntimeError("Failed to decode audio.") with the kind of failure: `status` is the indexer's
    negative AT_E_FLAC_* code or the decoder's positive AT_FLAC_* kind; `unsupported` = a stream this decoder does not
    read (Ogg-FLAC, 32-bit samples), which another decoder might."""

    def __init__(self, status):
        super().__init__("Failed to decode audio.")
        self.status = int(status)
        self.unsupported = self.status == -8      # AT_E_FLAC_UNSUPPORTED


def _flac_bytes(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    try:
        with open(src, "rb") as f:
            return f.read()
    except OSError:
        return b""


def load_flac_batch(paths, backend=None):
    """torchaudio.load for many .flac files (paths, or the files' bytes) in one device decode: per file, in order,
    (float32 [C, L] device tensor, sample_rate), or None for a file that could not be decoded; the kinds of the
    failures are left in backend.flac_status."""
    be = backend or default_backend()
    return be.flac_decode([_flac_bytes(p) for p in paths])


def load_flac(path_or_bytes, backend=None):
    """torchaudio.load(path) for a .flac file, decoded on the device: (float32 [C, L] device tensor, sample_rate).
    Any failure raises RuntimeError("Failed to decode audio."), the error the reference skips."""
    be = backend or default_backend()
    res = be.flac_decode([_flac_bytes(path_or_bytes)])[0]
    if res is None:
        raise FlacDecodeError(be.flac_status[0])
    return res


class LogMelSpectrogram:
    """MelSpectrogram(sample_rate, n_mels, n_fft, hop_length) followed by AmplitudeToDB(), fused.

    __call__(waveform [..., L]) -> [..., n_mels, T] float32 in dB (torchaudio's layout).
    n_fft: any even size from 64 to 4096 (400, torchaudio's own default, included); odd sizes are rejected."""

    def __init__(self, sample_rate=22050, n_fft=512, hop_length=128, n_mels=64, fb=None, backend=None):
        self.sample_rate, self.n_fft, self.hop_length, self.n_mels = sample_rate, n_fft, hop_length, n_mels
        self.backend = backend or default_backend()
        self.fb = None if fb is None else self.backend._f32(fb)

    def to(self, device):  # torchaudio-style chaining; the backend already pins the device
        return self

    def __call__(self, waveform):
        be = self.backend
        w = be._f32(waveform)
        lead = w.shape[:-1]
        out = be.logmel(w.reshape(-1, w.shape[-1]), self.sample_rate, self.n_fft, self.hop_length,
                        self.n_mels, fb=self.fb)
        return out.reshape(*lead, self.n_mels, out.shape[-1])

    def batch(self, waveforms, sample_rates=None, normalize=False):
        """Clips of any length, channel count and sample rate -> a list of [n_mels, T_i] dB spectrograms in input order,
        views of one flat device tensor; None where a clip is too short for the reflect padding (its length at
        self.sample_rate <= n_fft / 2).  waveforms: [C_i, L_i] or [L_i] tensors; sample_rates: one per clip (default:
        all at self.sample_rate).  Stereo is mixed to mono and other rates are resampled to self.sample_rate, with the
        bits of torch.mean and Resample per clip, in one launch per rate pair present and one log-mel launch
        (HipBackend.frontend_ragged).  normalize: every spectrogram scaled to (spec - min) / (max - min), the
        reference's normalize_spectrogram, in the same log-mel call.  self.last_bad: device int32 per clip, non-zero
        where its spectrogram (the scaled one under normalize: a constant clip gives 0 / 0) holds a NaN or Inf."""
        be = self.backend
        rates = self.sample_rate if sample_rates is None else sample_rates
        out, T, first, self.last_bad = be.frontend_ragged(waveforms, rates, self.sample_rate, self.n_fft, self.hop_length,
                                                          self.n_mels, fb=self.fb, minmax=normalize)
        m = self.n_mels
        return [None if T[i] == 0 else out[m * int(first[i]): m * (int(first[i]) + int(T[i]))].view(m, int(T[i]))
                for i in range(len(T))]

    def frames(self, waveform, l2norm=False):
        """[n_clips, L] -> frame-major [n_clips*T, n_mels] (optionally row-normalised): the matrix
        ClusterCreator / SpecTokenizer build from the .npy files, without the round trip."""
        be = self.backend
        return be.logmel(be._f32(waveform), self.sample_rate, self.n_fft, self.hop_length, self.n_mels,
                         fb=self.fb, frame_major=True, l2norm=l2norm)


class MFCC:
    """torchaudio.transforms.MFCC(sample_rate, n_mfcc, dct_type, norm, log_mels, melkwargs) on the device, with
    ComputeDeltas folded in: log-mel (LogMelSpectrogram's kernels), the per-clip top_db clamp of AmplitudeToDB, the
    DCT-II and `deltas` orders of time differences (0, 1 or 2; win_length as in ComputeDeltas, mode "replicate") in one
    kernel behind the log-mel call (HipBackend.mfcc, at_mfcc_f32; the arithmetic contract: DESIGN.md section 6k).

    __call__(waveform [..., L]) -> [..., D, T], D = n_mfcc * (1 + deltas), feature o * n_mfcc + k for order o.
    top_db=None, deltas=0 is the DCT of exactly what LogMelSpectrogram returns.  top_db clamps every clip at its OWN
    maximum - top_db (torchaudio takes one maximum over a whole [B, L] batch; the reference calls its transforms clip by
    clip).  dct: the caller's table [n_mels, n_mfcc], e.g. torchaudio.functional.create_dct's, in place of the
    library's, which evaluates the cosines in double.  dct_type other than 2 raises ValueError as torchaudio does;
    log_mels=True raises NotImplementedError (the log-mel kernels store dB only).
    A width with D % 4 != 0 (13 + delta + delta-delta = 39) sends the nearest-centroid searches down their general
    paths; 40, or 13 and a zero column, would take the 16-byte ones.  Padding is the caller's business."""

    def __init__(self, sample_rate=22050, n_mfcc=40, n_fft=512, hop_length=128, n_mels=64, dct_type=2, norm="ortho",
                 log_mels=False, top_db=80.0, deltas=0, win_length=5, dct=None, fb=None, backend=None):
        if dct_type != 2:
            raise ValueError(f"DCT type not supported: {dct_type}")
        if log_mels:
            raise NotImplementedError("log_mels=True: the log-mel kernels store dB only")
        if norm not in ("ortho", None):
            raise ValueError('norm must be "ortho" or None')
        if not 1 <= n_mfcc <= n_mels:
            raise ValueError("Cannot select more MFCC coefficients than # mel bins")
        if deltas not in (0, 1, 2):
            raise ValueError(f"deltas must be 0, 1 or 2, got {deltas}")
        if win_length < 3 or win_length % 2 == 0:
            raise ValueError(f"win_length must be odd and >= 3, got {win_length}")
        if top_db is not None and not top_db >= 0:
            raise ValueError("top_db must be positive value")
        self.sample_rate, self.n_fft, self.hop_length, self.n_mels = sample_rate, n_fft, hop_length, n_mels
        self.n_mfcc, self.norm, self.top_db, self.deltas, self.win_length = n_mfcc, norm, top_db, deltas, win_length
        self.D = n_mfcc * (1 + deltas)
        self.backend = be = backend or default_backend()
        self.fb = None if fb is None else be._f32(fb)
        self.dct = None if dct is None else be._f32(dct)
        if self.dct is not None and tuple(self.dct.shape) != (n_mels, n_mfcc):
            raise ValueError(f"dct must be [n_mels, n_mfcc] = [{n_mels}, {n_mfcc}], got {tuple(self.dct.shape)}")
        self.last_bad = None

    def to(self, device):
        return self

    def of_rows(self, rows, n_frames, frame_major=True):
        """The features of log-mel rows [n, n_mels] that are already on the device (HipBackend.mfcc's arguments)."""
        return self.backend.mfcc(rows, n_frames, n_mfcc=self.n_mfcc, dct=self.dct, orders=self.deltas,
                                 win_length=self.win_length, top_db=self.top_db, frame_major=frame_major, norm=self.norm)

    def _logmel_rows(self, waveform):
        be = self.backend
        w = be._f32(waveform)
        w2 = w.reshape(-1, w.shape[-1])
        rows = be.logmel(w2, self.sample_rate, self.n_fft, self.hop_length, self.n_mels, fb=self.fb, frame_major=True)
        return rows, w.shape[:-1], w2.shape[0]

    def __call__(self, waveform):
        rows, lead, n_clips = self._logmel_rows(waveform)
        T = rows.shape[0] // max(n_clips, 1)
        out = self.of_rows(rows, [T] * n_clips, frame_major=False)
        return out.reshape(*lead, self.D, T)

    def batch(self, waveforms, sample_rates=None):
        """LogMelSpectrogram.batch for these features: clips of any length, channel count and sample rate -> a list of
        [D, T_i] views of one flat device tensor, None where a clip is too short for the reflect padding.
        self.last_bad: the front end's per-clip flags (a NaN or Inf in the clip's log-mel)."""
        be = self.backend
        rates = self.sample_rate if sample_rates is None else sample_rates
        rows, T, first, self.last_bad = be.frontend_ragged(waveforms, rates, self.sample_rate, self.n_fft, self.hop_length,
                                                           self.n_mels, fb=self.fb, frame_major=True)
        out = self.of_rows(rows, T, frame_major=False)
        D = self.D
        return [None if T[i] == 0 else out[D * int(first[i]): D * (int(first[i]) + int(T[i]))].view(D, int(T[i]))
                for i in range(len(T))]

    def frames(self, waveform, l2norm=False):
        """[n_clips, L] -> frame-major [n_clips * T, D] (optionally row-normalised): the matrix Kmeans.train takes."""
        rows, _, n_clips = self._logmel_rows(waveform)
        out = self.of_rows(rows, [rows.shape[0] // max(n_clips, 1)] * n_clips)
        return self.backend.l2norm_rows(out) if l2norm else out


class ComputeDeltas:
    """torchaudio.transforms.ComputeDeltas(win_length, mode="replicate") on the device (HipBackend.deltas,
    at_deltas_f32): [..., F, T] -> the same shape.  The regression form of DESIGN.md section 6k, equal to torchaudio's
    in exact arithmetic; a constant input and T = 1 give exactly +0.  Any other mode raises ValueError."""

    def __init__(self, win_length=5, mode="replicate", backend=None):
        if mode != "replicate":
            raise ValueError(f'mode "{mode}" is not supported: only "replicate"')
        if win_length < 3 or win_length % 2 == 0:
            raise ValueError(f"win_length must be odd and >= 3, got {win_length}")
        self.win_length, self.mode = win_length, mode
        self.backend = backend or default_backend()

    def to(self, device):
        return self

    def __call__(self, specgram):
        be = self.backend
        x = be._f32(specgram)
        assert x.dim() >= 2, "ComputeDeltas: [..., F, T]"
        F, T = x.shape[-2], x.shape[-1]
        x3 = x.reshape(-1, F, T)
        rows = x3.transpose(1, 2).reshape(-1, F)
        out = be.deltas(rows, [T] * x3.shape[0], win_length=self.win_length)
        return out.reshape(x3.shape[0], T, F).transpose(1, 2).contiguous().reshape(x.shape)


class Resample:
    """torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults (sinc_interp_hann,
    lowpass_filter_width 6, rolloff 0.99).  __call__(waveform [..., L]) -> [..., ceil(L*new/orig)]
    on the device; equal rates return the input unchanged, as torchaudio does."""

    def __init__(self, orig_freq=16000, new_freq=16000, backend=None):
        if int(orig_freq) != orig_freq or int(new_freq) != new_freq:
            raise ValueError("Frequencies must be of integer type to ensure quality resampling computation.")
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        if self.orig_freq <= 0 or self.new_freq <= 0:
            raise ValueError("Original frequency and desired frequecy should be positive")
        self.backend = backend or default_backend()

    def to(self, device):
        return self

    def __call__(self, waveform):
        if self.orig_freq == self.new_freq:
            return waveform
        be = self.backend
        w = be._f32(waveform)
        lead = w.shape[:-1]
        out = be.resample(w.reshape(-1, w.shape[-1]), self.orig_freq, self.new_freq)
        return out.reshape(*lead, out.shape[-1])


class _Dist:
    """Thin view of torch.distributed for the sharded k-means (one process per GPU, RCCL).

    With the gloo backend (CPU tests, or several test ranks sharing one GPU) device tensors are
    staged through the host; with nccl (= RCCL) the collectives run on the device tensors."""

    def __init__(self, enabled, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.on = bool(enabled) and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
        self.group = group
        self.world = dist.get_world_size(group) if self.on else 1
        self.rank = dist.get_rank(group) if self.on else 0
        self.host_staged = self.on and dist.get_backend(group) == "gloo"

    def _all_reduce(self, t, op):
        if self.host_staged and t.device.type != "cpu":
            h = t.cpu()
            self.dist.all_reduce(h, op=op, group=self.group)
            t.copy_(h)
        else:
            self.dist.all_reduce(t, op=op, group=self.group)
        return t

    def _all_gather(self, t):
        """t [m] -> [world * m], rank order."""
        if self.host_staged and t.device.type != "cpu":
            h = t.cpu()
            out = torch.empty(self.world * h.numel(), dtype=h.dtype)
            self.dist.all_gather_into_tensor(out, h.reshape(-1), group=self.group)
            return out.to(t.device)
        out = torch.empty(self.world * t.numel(), dtype=t.dtype, device=t.device)
        self.dist.all_gather_into_tensor(out, t.reshape(-1), group=self.group)
        return out

    def all_gather_sizes(self, n_loc, device):
        if not self.on:
            return [n_loc]
        out = self._all_gather(torch.tensor([n_loc], dtype=torch.int64, device=device))
        return [int(v) for v in out.cpu()]

    def any_flag(self, flag: bool, device) -> bool:
        if not self.on:
            return flag
        t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=device)
        return bool(self._all_reduce(t, self.dist.ReduceOp.MAX).item())

    def all_gather_parts(self, part):
        """part [m] float32 -> [world, m], rank order."""
        if not self.on:
            return part.unsqueeze(0)
        return self._all_gather(part).view(self.world, part.numel())

    def reduce_in_rank_order(self, be, v):
        """v [m] float32 -> the sum over the ranks of v, added in ascending rank order, identical on every rank:
        all-to-all of the ranks' slices, ordered local sum of the slice this rank owns (at_sum_parts_f32), all-gather
        of the reduced slices.  Moves 2 (N-1)/N m floats per rank where the all-gather of whole partials moves
        (N-1) m -- the form for large tables (BASELINE.json's configs[4]: 8.45 MB per partial)."""
        if not self.on:
            return v
        w, m = self.world, v.numel()
        chunk = -(-m // w)
        chunk = (chunk + 3) // 4 * 4
        host = self.host_staged and v.device.type != "cpu"
        src = torch.zeros(w * chunk, dtype=v.dtype, device="cpu" if host else v.device)
        src[:m] = v.cpu() if host else v
        recv = torch.empty_like(src)
        self.dist.all_to_all_single(recv, src, group=self.group)          # recv[r] = rank r's copy of MY slice
        mine = be.sum_parts((recv.to(v.device) if host else recv).view(w, chunk))
        mine = mine.cpu() if host else mine
        out = torch.empty(w * chunk, dtype=v.dtype, device=mine.device)
        self.dist.all_gather_into_tensor(out, mine, group=self.group)
        out = out.to(v.device) if host else out
        return out[:m]

    def all_gather_f64(self, v):
        """v float64 [1] -> [world] in rank order."""
        if not self.on:
            return v.reshape(1)
        return self._all_gather(v.reshape(-1))

    def sum_bits(self, rows):
        """Exact merge of float32 rows of which exactly one rank holds a non-zero copy."""
        if not self.on:
            return rows
        bits = rows.view(torch.int32)
        return self._all_reduce(bits, self.dist.ReduceOp.SUM).view(torch.float32)

    def sum_f64(self, v):
        return self._all_reduce(v, self.dist.ReduceOp.SUM) if self.on else v


class _TrainingSet:
    """What one Kmeans.train() iterates over: `xs`, this rank's rows of the (global) training subsample of `ns` rows,
    -- sharded -- `pos`, their positions in it (ascending; None in a single process), and `ws`, the weights of the rows
    in `xs` (device float32 [rows of xs]; None for an unweighted training)."""

    def __init__(self, be, dist, xs, ns, pos, ws=None):
        self.be, self.dist, self.xs, self.ns, self.pos, self.ws = be, dist, xs, ns, pos, ws

    def rows_at(self, positions):
        """Rows of the (global) subsample at `positions` [m] -> device [m, d], on every rank."""
        be, dist, xs, pos = self.be, self.dist, self.xs, self.pos
        positions = np.asarray(positions, dtype=np.int64)
        if not dist.on:
            return be.gather_rows(xs, positions.astype(np.int32))
        out = be.zeros((len(positions), xs.shape[1]))
        want = be.from_host(positions)
        if pos.numel():
            j = torch.searchsorted(pos, want).clamp_(max=pos.numel() - 1)
            ok = pos[j] == want
            if bool(ok.any()):
                out[ok] = be.gather_rows(xs, j[ok].to(torch.int32).contiguous())
        return dist.sum_bits(out)


class _PrunedSweep:
    """The exact pruned search of one Kmeans.train() (d = 64 / 128: csrc/prune.hip) and the host schedule around it.

    The sweep skips by a spatial grouping of the centroids, `cperm`, computed on the host (group_rows_kd).  The
    grouping only decides how much the exact sweep can skip, never a result, so it may be of older centroids:
      - a cold start groups its initial centroids before it can begin, and regroups once they have settled
        (iteration 2);
      - a warm start begins with the grouping the previous train() ended with (`begin_with`) while the host regroups
        the new initial centroids beside the first iterations (`regroup`; not when it continues from that training's
        own result: the grouping is of centroids a few iterations older than these, nothing to redo);
      - a last regrouping near the end (late_due) is what the next warm start and the tokeniser's index begin with.
    A regrouping runs on the helper thread (_grouper) and is taken up by the first search queued after it is done.

    The host queues an iteration several times faster than the device runs it.  Left alone it would be a whole
    training ahead, and a regrouping -- which needs the device to have reached the centroids it groups, plus ~3 ms
    of host work -- would arrive after the host had queued every iteration that could have used it.  So the host
    stays at most AHEAD iterations ahead (waiting on an event that many iterations old: the device always has
    queued work) and measures the device's iteration time, `iter_ms`, from those events."""

    AHEAD = 3
    # what the path calls on a backend beyond the dense path's methods and HostHelpers' defaults
    NEEDS = ("assign_pruned", "assign_c2f", "group_min_dist", "group_means", "group_neighbours", "visit_order",
             "visit_order_beside", "sum_beside", "centroid_accum_join", "to_host_async", "record_event_timed")

    @classmethod
    def applies(cls, be, d, k, rows) -> bool:
        return (all(hasattr(be, name) for name in cls.NEEDS) and d in (64, 128) and k >= 1024 and (k + 31) // 32 <= 512
                and rows >= 4096)

    def __init__(self, be, k, niter, cent, cold, begin_with=None, regroup=False):
        self.be, self.k, self.niter, self.cold = be, k, niter, cold
        self.regrouping = None   # host grouping of newer centroids, under way on the helper thread
        self.regrouping_is_late = False
        self.paced = collections.deque()
        self.iter_ms = self.last_done = None
        if begin_with is None:
            self.cperm = be.from_host(be.group_rows_kd(be.to_host(cent)))
        else:
            self.cperm = begin_with
            if regroup:
                self.regrouping = self._regroup_beside(cent)

    def _regroup_beside(self, c):
        """Host grouping of the centroids `c` on the helper thread; the copy to the host is queued on the
        stream and waited for there, not here."""
        be = self.be
        h, ready = be.to_host_async(c)

        def job():
            ready.synchronize()
            return be.group_rows_kd(h.numpy())
        return _grouper().submit(job)

    def late_due(self, it) -> bool:
        """Whether the last regrouping should be under way at iteration `it`: from niter - 6 on, or earlier when the
        iterations left take the device no more than 4.5 ms (short iterations, a shard of an N-GPU run: submitted
        early enough to be finished when the last iteration is), never in the first half, never below 10 iterations."""
        niter = self.niter
        if niter < 10 or it < niter // 2:
            return False
        return it >= niter - 6 or (self.iter_ms is not None and (niter - it) * self.iter_ms <= 4.5)

    def search(self, it, xs, cent, vorder):
        """Queues iteration `it`'s exact search over the centroids `cent` -> (ids, dis).  vorder: the visiting order
        made from the previous iteration's answer (Kmeans._accumulate), None in iteration 0."""
        be = self.be
        if self.regrouping is not None and self.regrouping.done():
            self.cperm = be.from_host_async(self.regrouping.result())   # (the small table goes up without draining the stream)
            self.regrouping = None
        elif (it == 2 and self.cold and self.regrouping is None) or (self.late_due(it) and not self.regrouping_is_late):
            # cold start: regroup once the centroids have settled (taken up when the host is done); near the end:
            # for the next warm start and the tokeniser (replaces one still under way: these centroids are newer)
            self.regrouping_is_late = self.late_due(it)
            self.regrouping = self._regroup_beside(cent)
        dmin = be.group_min_dist(cent, self.cperm)
        if vorder is None:   # no previous assignment yet: coarse-to-fine exact search
            gnbr = be.group_neighbours(be.group_means(cent, self.cperm), 8)
            return be.assign_c2f(xs, cent, self.cperm, dmin, gnbr)
        return be.assign_pruned(xs, cent, vorder, self.cperm, dmin, image_current=True)

    def iteration_queued(self):
        """Behind everything an iteration queues: marks it with an event and waits for the iteration AHEAD before."""
        self.paced.append(self.be.record_event_timed())
        if len(self.paced) > self.AHEAD:
            done = self.paced.popleft()
            done.synchronize()
            if self.last_done is not None:
                self.iter_ms = self.last_done.elapsed_time(done)
            self.last_done = done

    def final_grouping(self):
        """The grouping the training ends with: the late regrouping, submitted early enough to be done or about to be
        (waits for it), else any that is done, else the one in use."""
        if self.regrouping is not None and (self.regrouping.done() or self.regrouping_is_late):
            self.cperm = self.be.from_host_async(self.regrouping.result())
        return self.cperm


class Kmeans:
    """faiss.Kmeans(d, k, niter=, verbose=, gpu=) for the reference's use (cluster_creator.py:42-48).

    ClusteringParameters are FAISS's defaults: nredo=1, seed=1234, max_points_per_centroid=256,
    min_points_per_centroid=39, no int / frozen centroids.  Each train() call is one
    faiss Clustering::train: subsample to k*256 rows with rand_perm(n, seed), initialise from
    `init_centroids` or from rand_perm(n_sub, seed+1), then niter x {nearest centroid, objective,
    ascending-index centroid sums, 1/count, split_clusters}.

    spherical=True is faiss' spherical k-means: the initial centroids are re-normalised (fvec_renorm_L2), every
    search is the inner-product search of IndexFlatIP (the objective is the sum of the products and grows), the
    centroids are re-normalised behind split_clusters in every iteration, and `index` is an IndexFlatIP.  Every
    iteration is one dense sweep: the pruned, hinted and filtered sweeps are exact for the L2 expression only.  It
    needs a backend with assign_ip() and renorm_rows() (else NotImplementedError).

    distributed=True (and torch.distributed initialised): `x` is this rank's block of the global
    row-concatenation in rank order; the result is identical on every rank.

    train(x, weights=w) is faiss' weighted training (`weights` is KEYWORD-ONLY here, faiss takes it as the second
    positional argument: an existing train(x, c) keeps its meaning).  The rows and their weights are subsampled
    together; initial centroids, the search and the per-iteration objective (the UNWEIGHTED sum of the returned
    distances) do not look at the weights; the centroid of a cluster is sum_i w_i x_i * (1 / sum_i w_i), both sums taken
    in ascending row order -- s <- fmaf(x_i, w_i, s) and s <- s + w_i from +0 --, and the weight sums stand where the
    member counts stood: in hassign, in the imbalance factor and in split_clusters, which re-seeds every cluster whose
    weight sum is 0.  All weights 1.0 give the bits of weights=None.  Weights are in units of "one point": with a
    weight sum of at most k the repair of an empty cluster finds no donor and the statistics raise RuntimeError.
    It needs a backend with centroid_accum_weighted() (else NotImplementedError, at the call).
    """

    def __init__(self, d, k, niter=20, verbose=False, gpu=True, seed=1234, max_points_per_centroid=256,
                 min_points_per_centroid=39, distributed=False, process_group=None, backend=None, spherical=False,
                 **kwargs):
        unsupported = {kk: v for kk, v in kwargs.items() if kk not in ("nredo",) or v != 1}
        if unsupported:
            raise NotImplementedError(f"Kmeans: unsupported ClusteringParameters {sorted(unsupported)}")
        self.spherical = bool(spherical)
        self.d, self.k, self.niter, self.verbose = int(d), int(k), int(niter), bool(verbose)
        self.gpu = gpu  # accepted for signature compatibility; this implementation is GPU-only
        self.seed = int(seed)
        self.max_points_per_centroid = int(max_points_per_centroid)
        self.min_points_per_centroid = int(min_points_per_centroid)
        self.backend = backend or default_backend()
        if self.spherical and not (hasattr(self.backend, "assign_ip") and hasattr(self.backend, "renorm_rows")):
            raise NotImplementedError("Kmeans: spherical=True needs a backend with assign_ip() and renorm_rows()")
        self._dist_enabled, self._group = distributed, process_group
        self.centroids_device = None   # [k, d] device tensor after train(); `.centroids` is its numpy copy (lazy)
        self._centroids_host = None
        self._iteration_stats, self._stats_pending = [], None
        self._last_assign = None            # ids of the last iteration's search (this rank's training rows)
        self._perm_cache = OrderedDict()    # _subsample_perm
        self._cperm_cache = None            # ((k, d), the grouping the last pruned train() ended with)
        self._grouping_of_result = None     # that grouping, until _finish has remembered it for the result
        self.index = None
        self.phase_seconds = None
        self.prune = True  # exact pruning of Lloyd iterations 2..niter (d = 64 / 128 only)
        self.order_beside = True   # the visiting-order sort on a stream of its own (A/B aid)
        self.exchange = "auto"     # "gather" | "scatter" | "auto": how the per-iteration partials are combined (see _exchange)

    # ------------------------------------------------------------------------------------
    def train(self, x, init_centroids=None, sync=True, check_finite=True, *, weights=None):
        """-> final objective (float), like faiss.  sync=False returns None without waiting for the device:
        centroids_device is valid in stream order, `.centroids` / `.obj` / `.iteration_stats` wait when read.
        check_finite=False skips faiss' NaN/Inf scan of x (a host round trip) for callers that have made it.

        weights (keyword-only): one weight per row of `x` -- [n], numpy or tensor, host or device, any float dtype,
        converted as x is; this rank's block when distributed -- for the weighted training the class describes.  A
        wrong length or ndim raises ValueError; with check_finite so does a NaN, infinite or negative weight (one more
        host read), without it nothing is read and the formula is followed.  None: the unweighted training, the same
        backend calls in the same order as before the argument existed."""
        be, k, d, niter, spherical = self.backend, self.k, self.d, self.niter, self.spherical
        if weights is not None and not hasattr(be, "centroid_accum_weighted"):
            raise NotImplementedError("Kmeans.train: weights need a backend with centroid_accum_weighted()")
        dist = _Dist(self._dist_enabled, self._group)
        ts = self._training_set(x, dist, check_finite, weights)
        xs, ns = ts.xs, ts.ns
        self._stats_pending = None
        self._iteration_stats = []
        if ns == k:  # faiss corner case: the training set becomes the centroids
            cent = ts.rows_at(np.arange(k))
            self._iteration_stats.append(dict(obj=0.0, time=0.0, time_search=0.0, imbalance_factor=1.0, nsplit=0))
            return self._finish(cent, sync)

        if init_centroids is not None:
            cent = be._f32(init_centroids).clone()
            assert tuple(cent.shape) == (k, d), f"init_centroids must be [{k}, {d}]"
        else:
            cent = ts.rows_at(be.rand_perm_prefix(ns, self.seed + 1, k))
        if spherical:
            cent = be.renorm_rows(cent)

        # ---- Lloyd iterations -------------------------------------------------------------
        # Nothing below waits for the device: empty clusters are repaired by a device kernel (same draws, same
        # bits as faiss' host loop) and {objective, imbalance, nsplit} of every iteration stay in two small device
        # arrays that are read once, after the last iteration (or per iteration when verbose).
        stats_dev = be.zeros((max(niter, 1), 2), torch.float64)
        nsplit_dev = be.zeros((max(niter, 1),), torch.int32)
        t0 = time.time()
        prof = self.phase_seconds  # None, or a dict that collects per-phase wall time (debug aid)

        def lap(name, t_prev):
            if prof is None:
                return t_prev
            be.synchronize()
            now = time.perf_counter()
            prof[name] = prof.get(name, 0.0) + (now - t_prev)
            return now

        # Iterations after the first reuse the previous assignment as a guess.  With d = 64/128 the
        # sweep is also pruned (exact: see csrc/prune.hip): `sweep` is that path's state, None without it.
        sweep = self._pruned_sweep(xs, cent, init_centroids)
        ids = dis = order = vorder = None
        for it in range(niter):
            tp = time.perf_counter()
            if sweep is not None:
                ids, dis = sweep.search(it, xs, cent, vorder)
            elif spherical:   # one dense inner-product sweep per iteration; `dis` holds the products
                ids, dis = be.assign_ip(xs, cent)
            elif ids is None:
                ids, dis = be.assign(xs, cent)
            else:  # same answer, guided by the previous assignment and its member-list order
                ids, dis = be.assign_hinted(xs, cent, ids, order)
            tp = lap("assign", tp)
            part, order, vorder = self._accumulate(xs, ids, dis, pruned=sweep is not None, last=it + 1 == niter, ws=ts.ws)
            tp = lap("accumulate", tp)
            parts, objs = self._exchange(dist, part)
            cent, hassign = be.centroid_finalize(parts, k, d)
            # statistics + repair of empty clusters (HipBackend: two single-workgroup passes, one launch)
            be.lloyd_stats_split(hassign, cent, ns, nsplit_dev[it:it + 1], parts, stats_dev[it], objs=objs)
            if spherical:
                cent = be.renorm_rows(cent)
            tp = lap("exchange+finalize+split", tp)
            if sweep is not None:
                sweep.iteration_queued()
        self._last_assign = ids
        self._stats_pending = (stats_dev[:niter], nsplit_dev[:niter], t0)
        if self.verbose:   # faiss' per-iteration lines, printed once the iterations are through (no wait inside the loop)
            for it, st in enumerate(self.iteration_stats):
                print(f"  Iteration {it} ({st['time']:.2f} s, search {st['time_search']:.2f} s): "
                      f"objective={st['obj']:g} imbalance={st['imbalance_factor']:.3f} nsplit={st['nsplit']}", flush=True)
        if sweep is not None:
            self._grouping_of_result = sweep.final_grouping()
            self._cperm_cache = ((k, d), self._grouping_of_result)
        return self._finish(cent, sync)

    # -- the pieces of train() ----------------------------------------------------------------
    def _training_set(self, x, dist, check_finite, weights=None) -> _TrainingSet:
        """faiss' input checks and subsample_training_set on this rank's rows `x` (and their weights)."""
        be, k, d = self.backend, self.k, self.d
        if isinstance(x, np.ndarray):
            assert x.flags.c_contiguous, "x must be C-contiguous"  # faiss asserts the same
        x = be._f32(x)
        assert x.dim() == 2 and x.shape[1] == d, f"expected [n, {d}], got {tuple(x.shape)}"
        n_loc = x.shape[0]
        w = None
        if weights is not None:
            if not isinstance(weights, (np.ndarray, torch.Tensor)):
                weights = np.asarray(weights)
            if weights.ndim != 1 or weights.shape[0] != n_loc:
                raise ValueError(f"weights must be [{n_loc}], one per row of x, got {tuple(weights.shape)}")
            w = be._f32(weights)
        sizes = dist.all_gather_sizes(n_loc, be.device)
        off = sum(sizes[:dist.rank])
        n = sum(sizes)
        if n < k:
            raise RuntimeError(f"Error: 'nx >= k' failed: Number of training points ({n}) should be at "
                               f"least as large as number of clusters ({k})")
        if check_finite and dist.any_flag(be.any_nonfinite(x) if n_loc else False, be.device):
            raise RuntimeError("Error: 'std::isfinite(x_in[i])' failed: input contains NaN's or Inf's")
        if w is not None and check_finite:
            # the library's own check (faiss makes none): sqrt(w) is finite exactly for the finite weights >= 0 (-0 included)
            if dist.any_flag(be.any_nonfinite(torch.sqrt(w)) if n_loc else False, be.device):
                raise ValueError("weights must be finite and not negative")

        if n > k * self.max_points_per_centroid:
            ns = k * self.max_points_per_centroid
            if self.verbose:
                print(f"Sampling a subset of {ns} / {n} for training")
            perm = self._subsample_perm(n, ns)      # device int32 [ns]: faiss' rand_perm(n, seed)[:ns]

            def gathered(rows):   # the weights follow the rows: the same positions of the same permutation
                return None if w is None else be.gather_rows(w.reshape(-1, 1), rows).reshape(-1)

            if not dist.on:
                return _TrainingSet(be, dist, be.gather_rows(x, perm), ns, None, gathered(perm))
            mine = (perm >= off) & (perm < off + n_loc)
            pos = torch.nonzero(mine).reshape(-1)              # subsample positions this rank owns (ascending)
            rows = (perm[mine] - off).to(torch.int32).contiguous()
            return _TrainingSet(be, dist, be.gather_rows(x, rows), ns, pos, gathered(rows))
        if n < k * self.min_points_per_centroid:
            print(f"WARNING clustering {n} points to {k} centroids: please provide at least "
                  f"{k * self.min_points_per_centroid} training points", file=sys.stderr)
        pos = off + torch.arange(n_loc, dtype=torch.int64, device=x.device) if dist.on else None
        return _TrainingSet(be, dist, x, n, pos, w)

    def _pruned_sweep(self, xs, cent, init_centroids):
        """The state of the exact pruned sweep over this train(), or None where the sweep is off or does not apply."""
        k, d = self.k, self.d
        if not (self.prune and not self.spherical and _PrunedSweep.applies(self.backend, d, k, xs.shape[0])):
            return None
        cached = self._cperm_cache
        if init_centroids is None or cached is None or cached[0] != (k, d):
            return _PrunedSweep(self.backend, k, self.niter, cent, cold=init_centroids is None)
        own_result = init_centroids is self.centroids_device or init_centroids is self._centroids_host
        return _PrunedSweep(self.backend, k, self.niter, cent, cold=False, begin_with=cached[1], regroup=not own_result)

    def _accumulate(self, xs, ids, dis, pruned, last, ws=None):
        """Queues this rank's packed partial of one iteration (HostHelpers.part_layout: centroid sums, counts and the
        objective sum_i dis[i]) and the row order the next search wants -> (part, order, vorder): `order` is the
        member-list order assign_hinted takes, `vorder` the visiting order of the pruned sweep; the other is None.
        ws: the rows' weights; the partial then holds the weighted sums and, in the counts' place, the weight sums."""
        be, k = self.backend, self.k
        obj_off, part_len = be.part_layout(k, self.d)
        part = be.empty((part_len,))
        obj_view = part[obj_off:obj_off + 2].view(torch.float64)             # this rank's objective rides along
        if ws is not None:
            # Weighted: everything on the main stream, one call behind the other (the objective stays the unweighted sum).
            be.sum_f64(dis, out=obj_view)
            part, order = be.centroid_accum_weighted(xs, ws, ids, k, out=part, want_order=True)
            if not pruned:
                return part, order, None
            return part, None, (be.visit_order(ids, dis, k) if not last else None)
        if not pruned:
            be.sum_f64(dis, out=obj_view)
            part, order = be.centroid_accum(xs, ids, k, out=part, want_order=True)
            return part, order, None
        # The next iteration's visiting order depends on this assignment only: its sort runs behind the short-list
        # accumulation while the long lists are still being summed on the side stream (defer_join).
        if xs.shape[0] >= 96 * k and self.order_beside and not last:
            # a third stream, beside both accumulations: the visiting order of the next iteration and the objective
            vjoin = be.visit_order_beside(ids, dis, k, sum_out=obj_view)
            be.centroid_accum(xs, ids, k, out=part, defer_join=True)
            vorder = vjoin()
            be.centroid_accum_join()
            return part, None, vorder
        sjoin = be.sum_beside(dis, obj_view)      # beside the accumulation; joined before the partial is used
        if xs.shape[0] < 96 * k:
            # With few rows per cluster on this rank (sharded runs) a cluster fills a tile or two and sorting its
            # rows by distance buys nothing: the member-list order of the accumulation doubles as the visiting
            # order and the second sort of the iteration is dropped (measured: -8 % per iteration at 32 rows per cluster).
            part, vorder = be.centroid_accum(xs, ids, k, out=part, want_order=True, defer_join=True)
        else:
            be.centroid_accum(xs, ids, k, out=part, defer_join=True)
            vorder = be.visit_order(ids, dis, k) if not last else None
        be.centroid_accum_join()
        sjoin()
        return part, None, vorder

    def _exchange(self, dist, part):
        """This rank's packed partial -> (parts, objs) for centroid_finalize and lloyd_stats_split, both of which add
        in rank order.  Up to 4 MB: an all-gather of whole partials (one collective, (N-1) x the table per rank), the
        objectives riding along (objs None).  Above: all-to-all + ordered local sum + all-gather (2 (N-1)/N x the
        table) -- (N-1)/N of the partial out, the reduced table back, sums and counts added by at_sum_parts_f32 on the
        slice each rank owns -- and the objectives travel as N doubles."""
        be = self.backend
        obj_off, part_len = be.part_layout(self.k, self.d)
        scatter = dist.on and (self.exchange == "scatter" or (self.exchange == "auto" and part_len * 4 > (4 << 20)))
        if not scatter:
            return dist.all_gather_parts(part), None
        red = be.empty((1, part_len))
        red[0, :obj_off] = dist.reduce_in_rank_order(be, part[:obj_off])
        red[0, obj_off:] = 0.0
        objs = dist.all_gather_f64(part[obj_off:obj_off + 2].view(torch.float64))
        return red, objs.contiguous()

    # -- results ----------------------------------------------------------------------------
    def _subsample_perm(self, n, m):
        """faiss' rand_perm(n, seed)[:m] on the device.  A pure function of (n, seed, m); the file batches of one
        run (one Kmeans object, as in ClusterCreator.run) mostly share n, so the last two are kept."""
        key = (int(n), self.seed, int(m))
        cache = self._perm_cache
        hit = cache.get(key)
        if hit is None:
            hit = cache[key] = self.backend.rand_perm_prefix_device(n, self.seed, m)
            while len(cache) > 2:
                cache.popitem(last=False)
        return hit

    def queued_stats(self):
        """The statistics of the last train() while they are still on the device (None once they have been read, or if
        there are none): a handle for read_stats(), good beyond later train() calls (sync=False callers that train
        batch after batch and read everything at the end)."""
        return self._stats_pending

    def read_stats(self, handle):
        """queued_stats() handle -> that training's iteration_stats (waits for it)."""
        stats_dev, nsplit_dev, t0 = handle
        be = self.backend
        st, ns = be.to_host(stats_dev), be.to_host(nsplit_dev)     # (waits for the iterations queued so far)
        if (ns < 0).any():
            raise RuntimeError("Kmeans: split_clusters found no donor (every cluster has at most one point; with "
                               "weights: their sum is at most k -- weights are in units of one point)")
        el = time.time() - t0
        return [dict(obj=float(np.float32(st[i, 0])), time=el * (i + 1) / len(ns), time_search=el * (i + 1) / len(ns),
                     imbalance_factor=float(st[i, 1]), nsplit=int(ns[i])) for i in range(len(ns))]

    @property
    def iteration_stats(self):
        """faiss' ClusteringIterationStats of the last train() (read back from the device on first use; `time`
        and `time_search` are the elapsed time spread evenly, the iterations are not timed one by one)."""
        if self._stats_pending is not None:
            self._iteration_stats = self.read_stats(self._stats_pending)
            self._stats_pending = None
        return self._iteration_stats

    @property
    def obj(self):
        return np.array([s["obj"] for s in self.iteration_stats], dtype=np.float32)

    @property
    def centroids(self):
        """numpy [k, d], like faiss (copied from the device on first use)."""
        if self._centroids_host is None and self.centroids_device is not None:
            self._centroids_host = self.backend.to_host(self.centroids_device)
        return self._centroids_host

    def lend_grouping(self, table) -> None:
        """Offers the spatial grouping this object ended with to an IndexFlatL2 later filled with `table`
        (e.g. the normalised centroids a tokeniser loads): nearby rows stay nearby, and the grouping only
        ever decides how much the exact search skips."""
        cached = self._cperm_cache
        if cached is not None:
            be = self.backend
            table = be.to_host(table) if isinstance(table, torch.Tensor) else np.asarray(table)
            if table.shape == cached[0]:
                be.remember_grouping(table, cached[1])

    def _finish(self, cent, sync=True):
        self.centroids_device = cent
        self._centroids_host = None
        self.index = (IndexFlatIP if self.spherical else IndexFlatL2)(self.d, backend=self.backend)
        self.index.add(cent)
        if self._grouping_of_result is not None:
            # for the index a tokeniser later builds from these very centroids (needs their host copy: sync)
            if sync:
                self.backend.remember_grouping(self.centroids, self._grouping_of_result)
            self._grouping_of_result = None
        if not sync:
            return None
        st = self.iteration_stats
        return float(st[-1]["obj"]) if st else 0.0


_GROUPER = None


def _grouper():
    """One helper thread for the host-side spatial grouping (a C call that releases the GIL)."""
    global _GROUPER
    if _GROUPER is None:
        from concurrent.futures import ThreadPoolExecutor
        _GROUPER = ThreadPoolExecutor(max_workers=1, thread_name_prefix="at-grouping")
    return _GROUPER


class IndexFlatL2:
    """faiss.IndexFlatL2(d) with add / search(x, k) / reset / ntotal (spec_tokenizer.py:123-127,77).

    search(x, k) returns (D, I), [n, k] float32 / int64, row-major: numpy for host input, device tensors (on the
    caller's current stream) for device input.  Row i lists the k smallest (dis, j) in lexicographic order, with dis
    exactly at_assign_f32's value; only centroids with dis < +inf are listed (NaN never is), and the slots left over
    (k > ntotal, an empty index, NaN rows, rows whose distances all overflow) hold I = -1, D = +inf.  On finite rows
    column 0 equals search(x, 1) bit for bit.  Deviation from faiss: its heap starts from FLT_MAX rather than +inf, so
    its empty slots would read D = FLT_MAX.  k >= 2 needs a backend with knn() (else NotImplementedError); k < 1
    raises RuntimeError, as faiss does."""

    def __init__(self, d, backend=None):
        self.d = int(d)
        self.backend = backend or default_backend()
        self._c = None
        self._prune = None   # (cperm, dmin, gnbr) for the coarse-to-fine exact search, built lazily
        self.prune = True
        self.rows_coherent = True   # queries arrive as consecutive frames of clips (spec_tokenizer.py:66-78)

    @property
    def ntotal(self) -> int:
        return 0 if self._c is None else int(self._c.shape[0])

    def reset(self) -> None:
        self._c = None
        self._prune = None

    def add(self, c) -> None:
        c = self.backend._f32(c)
        assert c.dim() == 2 and c.shape[1] == self.d, f"expected [n, {self.d}]"
        self._c = c.clone() if self._c is None else torch.cat([self._c, c], 0)
        self._prune = None

    def assign(self, x, want_dist=True):
        """Device tensors in, (ids [n] int64, dis [n] float32 or None) out: the search itself.  Large
        searches against large tables go through the exact coarse-to-fine pruned sweep."""
        be = self.backend
        c = self._c
        k = c.shape[0]
        if (self.prune and hasattr(be, "assign_c2f") and self.d in (64, 128) and k >= 1024
                and (k + 31) // 32 <= 512 and x.shape[0] >= 65536):
            if self._prune is None:
                c_host = be.to_host(c)
                cperm = be.recall_grouping(c_host)
                if cperm is None or cperm.numel() != ((k + 31) // 32) * 32:
                    cperm = be.from_host(be.group_rows_kd(c_host))
                # 4 neighbour groups for the one-launch guess generator (measured: 1-4 equal, 8 is 6 % slower)
                self._prune = (cperm, be.group_min_dist(c, cperm), be.group_neighbours(be.group_means(c, cperm), 4))
            cperm, dmin, gnbr = self._prune
            return be.assign_c2f(x, c, cperm, dmin, gnbr, want_dist=want_dist, coherent=self.rows_coherent)
        if (self.prune and hasattr(be, "assign_unguided") and self.d in (64, 128) and 128 <= k < 1024 and x.shape[0] >= 65536
                and getattr(be, "switches", {}).get("filter", True)):
            # too few centroids to prune (configs[1]: k = 500), enough rows to pay for the set-up: the same fp16-split
            # filter, every group visited
            if self._prune is None:
                self._prune = (be.from_host(be.group_rows_kd(be.to_host(c))), None, None)
            return be.assign_unguided(x, c, want_dist=want_dist, cperm=self._prune[0])
        return be.assign(x, c, want_dist=want_dist)

    def search(self, x, k=1):
        if k < 1:
            raise RuntimeError(f"IndexFlatL2.search: k must be at least 1, got {k}")
        if k != 1:
            return self._search_k(x, int(k))
        host = _is_host(x)
        be = self.backend
        x = be._f32(x)
        assert x.dim() == 2 and x.shape[1] == self.d, f"expected [n, {self.d}]"
        if self._c is None:
            D = torch.full((x.shape[0], 1), float("inf"), device=be.device)
            I = torch.full((x.shape[0], 1), -1, dtype=torch.int64, device=be.device)
        else:
            ids, dis = self.assign(x)
            D, I = dis.unsqueeze(1), ids.unsqueeze(1)
        return (be.to_host(D), be.to_host(I)) if host else (D, I)

    def _search_k(self, x, k):
        be = self.backend
        if not hasattr(be, "knn"):
            raise NotImplementedError("IndexFlatL2.search: k > 1 needs a backend with knn()")
        host = _is_host(x)
        x = be._f32(x)
        assert x.dim() == 2 and x.shape[1] == self.d, f"expected [n, {self.d}]"
        if self._c is None:
            D = torch.full((x.shape[0], k), float("inf"), device=be.device)
            I = torch.full((x.shape[0], k), -1, dtype=torch.int64, device=be.device)
        else:
            I, D = be.knn(x, self._c, k)
        return (be.to_host(D), be.to_host(I)) if host else (D, I)


class IndexFlatIP:
    """faiss.IndexFlatIP(d) with add / search(x, 1) / reset / ntotal: the index of Kmeans(spherical=True).

    search(x, 1) returns (D, I), [n, 1] float32 / int64: numpy for host input, device tensors (on the caller's current
    stream) for device input.  I[i] is the lowest j with the largest inner product among the centroids whose product
    is > -inf (a NaN product is never listed, +inf is), D[i] that product, exactly at_assign_ip_f32's value.  Rows with
    nothing to list (NaN rows, an empty index) hold I = -1, D = -inf.  Deviation from faiss: its heap starts from
    -FLT_MAX rather than -inf, so its empty slots would read D = -FLT_MAX.  k < 1 raises RuntimeError, as faiss does;
    k > 1 raises NotImplementedError: the top k by inner product is csrc/knn.hip's per-lane list with the key order
    reversed, a follow-up to this class."""

    def __init__(self, d, backend=None):
        self.d = int(d)
        self.backend = backend or default_backend()
        self._c = None

    @property
    def ntotal(self) -> int:
        return 0 if self._c is None else int(self._c.shape[0])

    def reset(self) -> None:
        self._c = None

    def add(self, c) -> None:
        c = self.backend._f32(c)
        assert c.dim() == 2 and c.shape[1] == self.d, f"expected [n, {self.d}]"
        self._c = c.clone() if self._c is None else torch.cat([self._c, c], 0)

    def assign(self, x, want_dist=True):
        """Device tensors in, (ids [n] int64, ip [n] float32 or None) out: the search itself."""
        return self.backend.assign_ip(x, self._c, want_dist=want_dist)

    def search(self, x, k=1):
        if k < 1:
            raise RuntimeError(f"IndexFlatIP.search: k must be at least 1, got {k}")
        if k != 1:
            raise NotImplementedError("IndexFlatIP.search: k > 1 (the top k by inner product: knn.hip's list with the "
                                      "key order reversed) is not implemented")
        host = _is_host(x)
        be = self.backend
        x = be._f32(x)
        assert x.dim() == 2 and x.shape[1] == self.d, f"expected [n, {self.d}]"
        if self._c is None:
            D = torch.full((x.shape[0], 1), float("-inf"), device=be.device)
            I = torch.full((x.shape[0], 1), -1, dtype=torch.int64, device=be.device)
        else:
            ids, ip = self.assign(x)
            D, I = ip.unsqueeze(1), ids.unsqueeze(1)
        return (be.to_host(D), be.to_host(I)) if host else (D, I)


class ProductQuantizer:
    """faiss.ProductQuantizer(d, M, nbits=8) with train / compute_codes / decode: M codebooks of ksub = 256 words, one per
    sub-vector of dsub = d // M features (M tokens per frame; the reference does not call it).

    train(x): for m = 0 .. M-1 in order, codebook m is bit for bit the `centroids` of Kmeans(dsub, 256, niter=niter,
    seed=seed, max_points_per_centroid=..., backend=backend).train(xm), xm a contiguous copy of x[:, m*dsub:(m+1)*dsub]:
    faiss's default training mode, one Clustering per sub-space over an IndexFlatL2(dsub).  Every sub-space uses the same
    seed and so the same subsample permutation.  Kmeans's errors and its small-training-set warning pass through.

    compute_codes(x) -> uint8 [n, M] (numpy for host input, a device tensor on the caller's current stream for device
    input): codes[i, m] is IndexFlatL2(dsub) holding codebook m asked .search(xm, 1), at_assign_f32's contract exactly (the
    direct form when the call has n < 20 rows).  A sub-vector with no distance below +inf (a NaN or Inf in it, or
    overflow) gets code 0; the call then raises RuntimeError in faiss's words, unless check_finite=False, which returns
    the codes and skips the one host read.  return_distances=True also returns the winning distances, float32 [n, M]
    (+inf for such a sub-vector).  decode(codes) -> float32 [n, d], the codebook rows copied.

    A backend with pq_encode() / pq_decode() (HipBackend: csrc/pq.hip) does each call in one launch; any other backend
    composes one assign() per sub-space on the contiguous slice, and decodes by indexing.  nbits != 8 raises
    NotImplementedError (faiss bit-packs other widths)."""

    def __init__(self, d, M, nbits=8, niter=25, seed=1234, max_points_per_centroid=256, verbose=False, backend=None):
        d, M, nbits = int(d), int(M), int(nbits)
        if M < 1 or d < 1 or d % M != 0:
            raise ValueError(f"ProductQuantizer: the dimension d = {d} must be a multiple of the number of sub-quantisers M = {M}")
        if nbits != 8:
            raise NotImplementedError(f"ProductQuantizer: nbits = {nbits} (only 8-bit codes, one byte per sub-space, are implemented)")
        self.d, self.M, self.nbits = d, M, nbits
        self.dsub, self.ksub, self.code_size = d // M, 256, M
        self.niter, self.seed, self.verbose = int(niter), int(seed), bool(verbose)
        self.max_points_per_centroid = int(max_points_per_centroid)
        self.backend = backend or default_backend()
        self.centroids_device = None   # [M, ksub, dsub] device tensor after train() / set_centroids()
        self._centroids_host = None

    @property
    def is_trained(self) -> bool:
        return self.centroids_device is not None

    @property
    def centroids(self):
        """numpy [M, ksub, dsub] float32 (None before training)."""
        if self._centroids_host is None and self.centroids_device is not None:
            self._centroids_host = self.backend.to_host(self.centroids_device)
        return self._centroids_host

    def set_centroids(self, c) -> None:
        """Takes a ready [M, 256, dsub] table (host or device) without training."""
        c = self.backend._f32(c)
        want = (self.M, self.ksub, self.dsub)
        if tuple(c.shape) != want:
            raise ValueError(f"ProductQuantizer.set_centroids: expected {list(want)}, got {list(c.shape)}")
        self.centroids_device = c.clone()
        self._centroids_host = None

    def _rows(self, x, what):
        x = self.backend._f32(x)
        assert x.dim() == 2 and x.shape[1] == self.d, f"{what}: expected [n, {self.d}], got {tuple(x.shape)}"
        return x

    def _require_trained(self, what):
        if not self.is_trained:
            raise RuntimeError(f"ProductQuantizer.{what}: the quantiser is not trained (call train() or set_centroids())")

    def train(self, x) -> None:
        be = self.backend
        x = self._rows(x, "ProductQuantizer.train")
        books = []
        for m in range(self.M):
            km = Kmeans(self.dsub, self.ksub, niter=self.niter, verbose=self.verbose, seed=self.seed,
                        max_points_per_centroid=self.max_points_per_centroid, backend=be)
            km.train(x[:, m * self.dsub:(m + 1) * self.dsub].contiguous())
            books.append(km.centroids_device)
        self.centroids_device = torch.stack(books, 0).contiguous()
        self._centroids_host = None

    def compute_codes(self, x, return_distances=False, check_finite=True):
        self._require_trained("compute_codes")
        be = self.backend
        host = _is_host(x)
        x = self._rows(x, "ProductQuantizer.compute_codes")
        cb = self.centroids_device
        if hasattr(be, "pq_encode"):
            codes, dist, bad = be.pq_encode(x, cb, want_dist=return_distances)
        else:
            ids, dis = [], []
            for m in range(self.M):
                i_m, d_m = be.assign(x[:, m * self.dsub:(m + 1) * self.dsub].contiguous(), cb[m], want_dist=return_distances)
                ids.append(i_m)
                dis.append(d_m)
            ids = torch.stack(ids, 1) if ids else torch.zeros((x.shape[0], 0), dtype=torch.int64)
            bad = (ids < 0).any().reshape(1).to(torch.int32)
            codes = ids.clamp(min=0).to(torch.uint8)
            # (the assignment leaves +inf where it lists nothing)
            dist = torch.stack(dis, 1).contiguous() if return_distances else None
        if check_finite and x.shape[0] and int(bad.item()):
            raise RuntimeError("Error: 'std::isfinite(x_in[i])' failed: input contains NaN's or Inf's")
        if host:
            codes, dist = be.to_host(codes), (be.to_host(dist) if return_distances else None)
        return (codes, dist) if return_distances else codes

    def decode(self, codes):
        self._require_trained("decode")
        be = self.backend
        host = _is_host(codes)
        if isinstance(codes, np.ndarray):
            codes = torch.from_numpy(np.ascontiguousarray(codes))
        assert codes.dim() == 2 and codes.shape[1] == self.M and codes.dtype == torch.uint8, \
            f"ProductQuantizer.decode: expected uint8 [n, {self.M}]"
        cb = self.centroids_device
        if hasattr(be, "pq_decode"):
            out = be.pq_decode(codes, cb)
        else:
            idx = codes.to(torch.int64)
            out = torch.cat([cb[m][idx[:, m]] for m in range(self.M)], 1).contiguous()
        return be.to_host(out) if host else out


class IndexPQ:
    """faiss.IndexPQ(d, M, nbits=8) with train / add / search(x, k) / reconstruct / reset / ntotal: the frames are kept as
    the M code bytes of `pq`, an ops.ProductQuantizer built from the constructor's arguments (same errors for d % M and
    nbits), and searched without being decoded (not used by the reference).

    add(x) appends pq.compute_codes(x) on the device (check_finite passes through; the encoder's error is raised
    before anything is appended); add_codes(codes) appends a ready uint8 [n, M] array, host or device; `codes` is the
    device tensor [ntotal, M]; reset() drops the codes and keeps the codebooks.

    search(x, k) returns (D, I), [n, k] float32 / int64: numpy for host input, device tensors (on the caller's current
    stream) for device input.  The distance of query i to stored row r is the asymmetric one of faiss's default
    ST_PQ search -- the table T[i, m, j] = sum_f (x[i, m*dsub + f] - codebook[m, j, f])^2, always in the direct form (one
    fp32 subtraction, an ascending fmaf chain from +0), then T[i, 0, codes[r, 0]] + T[i, 1, codes[r, 1]] + ... added in
    ascending m, one fp32 addition each -- recalled from faiss, not verified against its output.  Row i lists the k
    smallest (dis, r) in lexicographic order, only rows with dis < +inf (NaN never is); the slots left over (ntotal <
    k, an empty index, a NaN or Inf in the query, overflow) hold I = -1, D = +inf: IndexFlatL2.search's conventions,
    its deviation from faiss's FLT_MAX included.  k < 1 raises RuntimeError, as faiss does; k > 128 and M > 64 raise
    NotImplementedError (the kernel keeps a query's tables and candidates in LDS; there is no path behind either
    limit), and so does a backend without pq_search(): torch arithmetic cannot restate the fmaf chain, so there is no
    composed route.  reconstruct_n(i0, n) / reconstruct(i) return pq.decode of the stored codes (numpy)."""

    MAX_M, MAX_K = 64, 128

    def __init__(self, d, M, nbits=8, niter=25, seed=1234, max_points_per_centroid=256, verbose=False, backend=None):
        self.pq = ProductQuantizer(d, M, nbits=nbits, niter=niter, seed=seed,
                                   max_points_per_centroid=max_points_per_centroid, verbose=verbose, backend=backend)
        if self.pq.M > self.MAX_M:
            raise NotImplementedError(f"IndexPQ: M = {self.pq.M} (at most {self.MAX_M} sub-quantisers are implemented)")
        self.backend = self.pq.backend
        if not hasattr(self.backend, "pq_search"):
            raise NotImplementedError("IndexPQ needs a backend with pq_search()")
        self.d, self.M = self.pq.d, self.pq.M
        self._codes = None

    @property
    def is_trained(self) -> bool:
        return self.pq.is_trained

    @property
    def ntotal(self) -> int:
        return 0 if self._codes is None else int(self._codes.shape[0])

    @property
    def codes(self):
        """The stored codes, a uint8 device tensor [ntotal, M]."""
        if self._codes is None:
            return self.backend.empty((0, self.M), torch.uint8)
        return self._codes

    def train(self, x) -> None:
        self.pq.train(x)

    def reset(self) -> None:
        self._codes = None

    def _append(self, codes) -> None:
        if isinstance(codes, np.ndarray):   # (a backend whose device is the host answers with numpy)
            codes = torch.from_numpy(np.ascontiguousarray(codes))
        assert codes.dim() == 2 and codes.shape[1] == self.M and codes.dtype == torch.uint8, \
            f"IndexPQ: expected uint8 codes [n, {self.M}]"
        codes = codes.to(self.backend.device).contiguous()
        self._codes = codes.clone() if self._codes is None else torch.cat([self._codes, codes], 0)

    def add(self, x, check_finite=True) -> None:
        if not self.is_trained:
            raise RuntimeError("IndexPQ.add: the index is not trained (call train() or pq.set_centroids())")
        x = self.pq._rows(x, "IndexPQ.add")   # (on the device: compute_codes then answers with a device tensor)
        self._append(self.pq.compute_codes(x, check_finite=check_finite))

    def add_codes(self, codes) -> None:
        self._append(codes)

    def search(self, x, k=1):
        k = int(k)
        if k < 1:
            raise RuntimeError(f"IndexPQ.search: k must be at least 1, got {k}")
        if k > self.MAX_K:
            raise NotImplementedError(f"IndexPQ.search: k = {k} (at most {self.MAX_K} neighbours are implemented)")
        if not self.is_trained:
            raise RuntimeError("IndexPQ.search: the index is not trained (call train() or pq.set_centroids())")
        be = self.backend
        host = _is_host(x)
        x = self.pq._rows(x, "IndexPQ.search")
        if self._codes is None:
            D = torch.full((x.shape[0], k), float("inf"), device=be.device)
            I = torch.full((x.shape[0], k), -1, dtype=torch.int64, device=be.device)
        else:
            I, D = be.pq_search(x, self.pq.centroids_device, self._codes, k)
        return (be.to_host(D), be.to_host(I)) if host else (D, I)

    def reconstruct_n(self, i0=0, n=-1):
        """float32 numpy [n, d]: the decoded rows i0 .. i0 + n - 1 (n = -1: to the end)."""
        i0, n = int(i0), int(n)
        if n < 0:
            n = self.ntotal - i0
        if i0 < 0 or n < 0 or i0 + n > self.ntotal:
            raise RuntimeError(f"IndexPQ.reconstruct_n: rows {i0} .. {i0 + n} of {self.ntotal}")
        out = self.pq.decode(self.codes[i0:i0 + n])
        return out if isinstance(out, np.ndarray) else self.backend.to_host(out)

    def reconstruct(self, i):
        return self.reconstruct_n(i, 1)[0]


class IndexIVFFlat:
    """faiss.IndexIVFFlat(quantizer, d, nlist) under L2 with train / add / add_core / search(x, k) / reset / ntotal /
    nprobe / list_sizes: the stored rows are kept grouped by the nearest centroid of `quantizer`, an ops.IndexFlatL2(d),
    and a query is compared only with the rows of the nprobe lists nearest to it (not used by the reference).  A
    trained vocabulary is a ready quantiser, and the token of a frame is its list number.

    is_trained is quantizer.ntotal == nlist: a quantiser that already holds nlist rows needs no training; any other
    non-zero ntotal raises RuntimeError.  train(x) does nothing when trained; otherwise it adds the centroids of
    Kmeans(d, nlist, niter=10, seed=1234, max_points_per_centroid=256) on x to the quantiser (niter = 10: faiss's
    level-1 default).

    add(x) appends rows with the ids ntotal, ntotal + 1, ...; the list of a row is quantizer.assign(x), the exact
    search the tokeniser makes (a row with a NaN or Inf in it gets no list).  add_core(x, precomputed_idx) takes the caller's int64 list numbers as they are (tokens
    already computed); values outside [-1, nlist) raise.  A row whose list is -1 (a NaN row, a row no centroid is
    listable for) counts in ntotal and sits in no list, as in faiss; add() with check_finite=True (the default) raises
    RuntimeError in faiss's words for such a row before anything is appended, check_finite=False skips that one host
    read.  Adding before training raises.  The searchable image is built at the first search after an add and cached;
    the raw rows are kept beside it (DESIGN.md section 6o says what that costs).  reset() drops the stored rows and
    keeps the quantiser.

    search(x, k) returns (D, I), [n, k] float32 / int64: numpy for host input, device tensors (on the caller's current
    stream) for device input.  The contract, the library's own:
      * the probed lists of query i are the ids in row i of backend.knn(x, centroids, min(nprobe, nlist)) -- at_knn_f32
        itself, its direct form for n < 20 included; a -1 slot is no list; only the set matters;
      * dis(i, r) between query i and stored row r is ALWAYS the expansion form of at_assign_f32, whatever n is: ip,
        |x|^2, |r|^2 ascending fmaf chains, (xn + rn) - 2*ip in one fma, the clamp v < 0 ? 0 : v (a NaN stays a NaN);
      * row i lists the k smallest (dis, id) in lexicographic order over the stored rows of its probed lists with
        dis < +inf; the slots left over hold I = -1, D = +inf (IndexFlatL2.search's conventions);
      * so with nprobe >= nlist, n >= 20 and no unlisted stored row the result equals
        IndexFlatL2(d).add(stored).search(x, k) bit for bit.
    nprobe (default 1): values above nlist act as nlist, values below 1 raise at search.  k < 1 raises RuntimeError,
    k > 32 NotImplementedError (the per-lane list of the kernel, as in IndexFlatL2's fused path; a larger k is a
    follow-up).  No remove_ids, add_with_ids, reconstruct or inner-product metric."""

    MAX_K = 32

    def __init__(self, quantizer, d, nlist, backend=None):
        self.d, self.nlist = int(d), int(nlist)
        if self.nlist < 1:
            raise ValueError(f"IndexIVFFlat: nlist = {nlist} (at least one list)")
        if not isinstance(quantizer, IndexFlatL2) or quantizer.d != self.d:
            raise ValueError(f"IndexIVFFlat: the quantizer must be an ops.IndexFlatL2({self.d})")
        self.quantizer = quantizer
        self.backend = backend or quantizer.backend
        for need in ("knn", "ivf_build", "ivf_search"):
            if not hasattr(self.backend, need):
                raise NotImplementedError(f"IndexIVFFlat needs a backend with {need}()")
        self.nprobe = 1
        self._x = None        # [ntotal, d] float32, the raw rows
        self._lists = None    # [ntotal] int64
        self._image = None    # backend.ivf_build's record, built lazily
        _ = self.is_trained

    @property
    def is_trained(self) -> bool:
        have = self.quantizer.ntotal
        if have not in (0, self.nlist):
            raise RuntimeError(f"IndexIVFFlat: the quantizer holds {have} rows, the index has nlist = {self.nlist} lists")
        return have == self.nlist

    @property
    def ntotal(self) -> int:
        return 0 if self._x is None else int(self._x.shape[0])

    @property
    def list_sizes(self):
        """int64 numpy [nlist]: the rows in every list (rows in no list are in none)."""
        sizes = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.backend.device)
        if self._lists is not None:
            at = torch.where(self._lists < 0, torch.full_like(self._lists, self.nlist), self._lists)
            sizes.scatter_add_(0, at, torch.ones_like(at))
        return self.backend.to_host(sizes[:self.nlist].contiguous())

    def train(self, x) -> None:
        if self.is_trained:
            return
        km = Kmeans(self.d, self.nlist, niter=10, seed=1234, max_points_per_centroid=256, backend=self.backend)
        km.train(self._rows(x, "IndexIVFFlat.train"))
        self.quantizer.add(km.centroids_device)

    def reset(self) -> None:
        self._x = self._lists = self._image = None

    def _rows(self, x, what):
        x = self.backend._f32(x)
        assert x.dim() == 2 and x.shape[1] == self.d, f"{what}: expected [n, {self.d}], got {tuple(x.shape)}"
        return x

    def _append(self, x, lists) -> None:
        self._x = x.clone() if self._x is None else torch.cat([self._x, x], 0)
        self._lists = lists.clone() if self._lists is None else torch.cat([self._lists, lists], 0)
        self._image = None

    def add(self, x, check_finite=True) -> None:
        if not self.is_trained:
            raise RuntimeError("IndexIVFFlat.add: the index is not trained (call train(), or hand it a full quantizer)")
        x = self._rows(x, "IndexIVFFlat.add")
        if x.shape[0] == 0:
            return
        lists, _ = self.quantizer.assign(x, want_dist=False)
        # at_assign_f32 clamps with fmaxf, which turns the NaN distances of a row with a NaN or Inf in it into 0 and
        # names centroid 0; the oracle, at_knn_f32 and this index list no centroid for such a row
        lists = torch.where(torch.isfinite(x).all(1), lists, torch.full_like(lists, -1))
        if check_finite and bool((lists < 0).any().item()):
            raise RuntimeError("Error: 'std::isfinite(x_in[i])' failed: input contains NaN's or Inf's")
        self._append(x, lists)

    def add_core(self, x, precomputed_idx) -> None:
        if not self.is_trained:
            raise RuntimeError("IndexIVFFlat.add_core: the index is not trained (call train(), or hand it a full quantizer)")
        x = self._rows(x, "IndexIVFFlat.add_core")
        if isinstance(precomputed_idx, np.ndarray):
            precomputed_idx = torch.from_numpy(np.ascontiguousarray(precomputed_idx))
        lists = torch.as_tensor(precomputed_idx)
        if lists.dtype != torch.int64 or lists.dim() != 1 or lists.shape[0] != x.shape[0]:
            raise ValueError(f"IndexIVFFlat.add_core: expected int64 list numbers [{x.shape[0]}]")
        if x.shape[0] == 0:
            return
        lists = lists.to(self.backend.device).contiguous()
        lo, hi = int(lists.min().item()), int(lists.max().item())
        if lo < -1 or hi >= self.nlist:
            raise RuntimeError(f"IndexIVFFlat.add_core: list numbers {lo} .. {hi} outside -1 .. {self.nlist - 1}")
        self._append(x, lists)

    def search(self, x, k=1):
        k = int(k)
        if k < 1:
            raise RuntimeError(f"IndexIVFFlat.search: k must be at least 1, got {k}")
        if k > self.MAX_K:
            raise NotImplementedError(f"IndexIVFFlat.search: k = {k} (at most {self.MAX_K} neighbours are implemented)")
        nprobe = int(self.nprobe)
        if nprobe < 1:
            raise RuntimeError(f"IndexIVFFlat.search: nprobe must be at least 1, got {nprobe}")
        if not self.is_trained:
            raise RuntimeError("IndexIVFFlat.search: the index is not trained (call train(), or hand it a full quantizer)")
        be = self.backend
        host = _is_host(x)
        x = self._rows(x, "IndexIVFFlat.search")
        if self._x is None or x.shape[0] == 0:
            D = torch.full((x.shape[0], k), float("inf"), device=be.device)
            I = torch.full((x.shape[0], k), -1, dtype=torch.int64, device=be.device)
        else:
            if self._image is None:
                self._image = be.ivf_build(self._x, self._lists, self.nlist)
            probes, _ = be.knn(x, self.quantizer._c, min(nprobe, self.nlist), want_dist=False)
            I, D = be.ivf_search(x, probes, self._image, k)
        return (be.to_host(D), be.to_host(I)) if host else (D, I)


class IndexIVFPQ:
    """faiss.IndexIVFPQ(quantizer, d, nlist, M, nbits=8) under L2 with train / add / add_core / search(x, k) /
    reconstruct / reset / ntotal / nprobe / list_sizes / codes: the stored rows are kept as the M code bytes of `pq`, an
    ops.ProductQuantizer(d, M, ...) built from the constructor's arguments (same errors for d % M and nbits), grouped by
    the nearest centroid of `quantizer`, an ops.IndexFlatL2(d), and a query meets only the codes of the nprobe lists
    nearest to it (not used by the reference).  The contract is the library's own, in the manner of IndexPQ and
    IndexIVFFlat: recalled, not verified against faiss output.

    is_trained is quantizer.ntotal == nlist (any other non-zero ntotal raises RuntimeError) and pq.is_trained.  train(x)
    first trains an empty quantiser as IndexIVFFlat.train does, then trains pq on x - c[assign(x)] (a device gather and
    one fp32 subtraction), or on x itself when by_residual is False.

    add(x) appends rows with the ids ntotal, ntotal + 1, ...; the list of a row is quantizer.assign(x), -1 for a row
    with a NaN or Inf in it, which counts in ntotal, sits in no list and is never found; with check_finite=True (the
    default) such a row raises RuntimeError in faiss's words before anything is appended.  add_core(x, precomputed_idx)
    takes the caller's int64 list numbers in [-1, nlist).  Row r of list l >= 0 stores pq.compute_codes(x[r] - c[l])
    (by_residual, one fp32 subtraction per feature) or pq.compute_codes(x[r]); a row of list -1 is encoded from a
    zero vector.  `codes` is the uint8 device tensor [ntotal, M] in id order, kept beside the grouped image (built
    at the first search after an add, and cached).  reset() keeps the quantiser and the codebooks.
    reconstruct_n(i0, n) / reconstruct(i) give pq.decode(codes), plus c[list] in one fp32 addition when by_residual,
    and NaN rows for list -1 (numpy).

    search(x, k) returns (D, I), [n, k] float32 / int64: numpy for host input, device tensors (on the caller's current
    stream) for device input:
      * the probed lists of query i are the ids in row i of backend.knn(x, centroids, min(nprobe, nlist)); a -1 slot
        is no list;
      * for query i and probed list l the query vector is q = x[i] - c[l] (one fp32 subtraction per feature) when
        by_residual, x[i] itself otherwise; the table is T[m, j] = sum_f (q[m*dsub + f] - codebook[m, j, f])^2 in
        IndexPQ's direct form (one subtraction, an ascending fmaf chain from +0), and a row r of list l has
        dis(i, r) = T[0, code[r, 0]] + T[1, code[r, 1]] + ..., one fp32 addition per step in ascending m.  The
        expansion form appears nowhere; faiss's precomputed-table decomposition of the residual distance is a
        different arithmetic and is not implemented;
      * row i lists the k smallest (dis, id) in lexicographic order over the stored rows of its probed lists with
        dis < +inf (NaN never is); the slots left over hold I = -1, D = +inf; a non-finite query lists nothing;
      * so with by_residual=False, nprobe >= nlist and no unlisted row the result equals IndexPQ.search(x, k) over
        the same codebooks and codes bit for bit, for every n.
    nprobe (default 1): values above nlist act as nlist, values below 1 raise at search.  k < 1 raises RuntimeError;
    k > 128, M > 64 and nlist > 2^24 raise NotImplementedError, and so does a backend without ivfpq_build() /
    ivfpq_search().  No inner-product metric, remove_ids, add_with_ids, polysemous codes or nbits != 8."""

    MAX_M, MAX_K, MAX_NLIST = 64, 128, 1 << 24

    def __init__(self, quantizer, d, nlist, M, nbits=8, by_residual=True, niter=25, seed=1234,
                 max_points_per_centroid=256, verbose=False, backend=None):
        self.d, self.nlist = int(d), int(nlist)
        if self.nlist < 1:
            raise ValueError(f"IndexIVFPQ: nlist = {nlist} (at least one list)")
        if self.nlist > self.MAX_NLIST:
            raise NotImplementedError(f"IndexIVFPQ: nlist = {nlist} (at most {self.MAX_NLIST} lists are implemented)")
        if not isinstance(quantizer, IndexFlatL2) or quantizer.d != self.d:
            raise ValueError(f"IndexIVFPQ: the quantizer must be an ops.IndexFlatL2({self.d})")
        self.quantizer = quantizer
        self.backend = backend or quantizer.backend
        self.pq = ProductQuantizer(d, M, nbits=nbits, niter=niter, seed=seed,
                                   max_points_per_centroid=max_points_per_centroid, verbose=verbose, backend=self.backend)
        if self.pq.M > self.MAX_M:
            raise NotImplementedError(f"IndexIVFPQ: M = {self.pq.M} (at most {self.MAX_M} sub-quantisers are implemented)")
        for need in ("knn", "ivfpq_build", "ivfpq_search"):
            if not hasattr(self.backend, need):
                raise NotImplementedError(f"IndexIVFPQ needs a backend with {need}()")
        self.M, self.by_residual = self.pq.M, bool(by_residual)
        self.nprobe = 1
        self._codes = None    # [ntotal, M] uint8, in id order
        self._lists = None    # [ntotal] int64
        self._image = None    # backend.ivfpq_build's record, built lazily
        _ = self.is_trained

    @property
    def is_trained(self) -> bool:
        have = self.quantizer.ntotal
        if have not in (0, self.nlist):
            raise RuntimeError(f"IndexIVFPQ: the quantizer holds {have} rows, the index has nlist = {self.nlist} lists")
        return have == self.nlist and self.pq.is_trained

    @property
    def ntotal(self) -> int:
        return 0 if self._codes is None else int(self._codes.shape[0])

    @property
    def codes(self):
        """The stored codes in id order, a uint8 device tensor [ntotal, M]."""
        if self._codes is None:
            return self.backend.empty((0, self.M), torch.uint8)
        return self._codes

    @property
    def list_sizes(self):
        """int64 numpy [nlist]: the rows in every list (rows in no list are in none)."""
        sizes = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.backend.device)
        if self._lists is not None:
            at = torch.where(self._lists < 0, torch.full_like(self._lists, self.nlist), self._lists)
            sizes.scatter_add_(0, at, torch.ones_like(at))
        return self.backend.to_host(sizes[:self.nlist].contiguous())

    def _rows(self, x, what):
        x = self.backend._f32(x)
        assert x.dim() == 2 and x.shape[1] == self.d, f"{what}: expected [n, {self.d}], got {tuple(x.shape)}"
        return x

    def _encoder_input(self, x, lists):
        """What the encoder sees of the rows x with the list numbers `lists`: x - c[list] (by_residual) or x, and a zero
        vector for a row of list -1."""
        out = x
        if self.by_residual:
            out = x - self.quantizer._c[lists.clamp(min=0)]
        return torch.where((lists < 0)[:, None], torch.zeros_like(out), out).contiguous()

    def train(self, x) -> None:
        x = self._rows(x, "IndexIVFPQ.train")
        if self.quantizer.ntotal != self.nlist:
            _ = self.is_trained   # (raises for a quantiser of another size)
            km = Kmeans(self.d, self.nlist, niter=10, seed=1234, max_points_per_centroid=256, backend=self.backend)
            km.train(x)
            self.quantizer.add(km.centroids_device)
        if self.by_residual:
            lists, _ = self.quantizer.assign(x, want_dist=False)
            x = (x - self.quantizer._c[lists.clamp(min=0)]).contiguous()
        self.pq.train(x)

    def reset(self) -> None:
        self._codes = self._lists = self._image = None

    def _append(self, x, lists, check_finite) -> None:
        codes = self.pq.compute_codes(self._encoder_input(x, lists), check_finite=check_finite)
        if isinstance(codes, np.ndarray):   # (a backend whose device is the host answers with numpy)
            codes = torch.from_numpy(np.ascontiguousarray(codes))
        codes = codes.to(self.backend.device).contiguous()
        self._codes = codes.clone() if self._codes is None else torch.cat([self._codes, codes], 0)
        self._lists = lists.clone() if self._lists is None else torch.cat([self._lists, lists], 0)
        self._image = None

    def add(self, x, check_finite=True) -> None:
        if not self.is_trained:
            raise RuntimeError("IndexIVFPQ.add: the index is not trained (call train(), or hand it a full quantizer and pq.set_centroids())")
        x = self._rows(x, "IndexIVFPQ.add")
        if x.shape[0] == 0:
            return
        lists, _ = self.quantizer.assign(x, want_dist=False)
        # (IndexIVFFlat.add: the assignment names centroid 0 for a row with a NaN or Inf in it; such a row gets no list)
        lists = torch.where(torch.isfinite(x).all(1), lists, torch.full_like(lists, -1))
        if check_finite and bool((lists < 0).any().item()):
            raise RuntimeError("Error: 'std::isfinite(x_in[i])' failed: input contains NaN's or Inf's")
        self._append(x, lists, check_finite)

    def add_core(self, x, precomputed_idx) -> None:
        if not self.is_trained:
            raise RuntimeError("IndexIVFPQ.add_core: the index is not trained (call train(), or hand it a full quantizer and pq.set_centroids())")
        x = self._rows(x, "IndexIVFPQ.add_core")
        if isinstance(precomputed_idx, np.ndarray):
            precomputed_idx = torch.from_numpy(np.ascontiguousarray(precomputed_idx))
        lists = torch.as_tensor(precomputed_idx)
        if lists.dtype != torch.int64 or lists.dim() != 1 or lists.shape[0] != x.shape[0]:
            raise ValueError(f"IndexIVFPQ.add_core: expected int64 list numbers [{x.shape[0]}]")
        if x.shape[0] == 0:
            return
        lists = lists.to(self.backend.device).contiguous()
        lo, hi = int(lists.min().item()), int(lists.max().item())
        if lo < -1 or hi >= self.nlist:
            raise RuntimeError(f"IndexIVFPQ.add_core: list numbers {lo} .. {hi} outside -1 .. {self.nlist - 1}")
        self._append(x, lists, False)

    def search(self, x, k=1):
        k = int(k)
        if k < 1:
            raise RuntimeError(f"IndexIVFPQ.search: k must be at least 1, got {k}")
        if k > self.MAX_K:
            raise NotImplementedError(f"IndexIVFPQ.search: k = {k} (at most {self.MAX_K} neighbours are implemented)")
        nprobe = int(self.nprobe)
        if nprobe < 1:
            raise RuntimeError(f"IndexIVFPQ.search: nprobe must be at least 1, got {nprobe}")
        if not self.is_trained:
            raise RuntimeError("IndexIVFPQ.search: the index is not trained (call train(), or hand it a full quantizer and pq.set_centroids())")
        be = self.backend
        host = _is_host(x)
        x = self._rows(x, "IndexIVFPQ.search")
        if self._codes is None or x.shape[0] == 0:
            D = torch.full((x.shape[0], k), float("inf"), device=be.device)
            I = torch.full((x.shape[0], k), -1, dtype=torch.int64, device=be.device)
        else:
            if self._image is None:
                self._image = be.ivfpq_build(self._codes, self._lists, self.nlist)
            probes, _ = be.knn(x, self.quantizer._c, min(nprobe, self.nlist), want_dist=False)
            I, D = be.ivfpq_search(x, probes, self.quantizer._c if self.by_residual else None, self.pq.centroids_device,
                                   self._image, k)
        return (be.to_host(D), be.to_host(I)) if host else (D, I)

    def reconstruct_n(self, i0=0, n=-1):
        """float32 numpy [n, d]: the decoded rows i0 .. i0 + n - 1 (n = -1: to the end), NaN for a row of list -1."""
        i0, n = int(i0), int(n)
        if n < 0:
            n = self.ntotal - i0
        if i0 < 0 or n < 0 or i0 + n > self.ntotal:
            raise RuntimeError(f"IndexIVFPQ.reconstruct_n: rows {i0} .. {i0 + n} of {self.ntotal}")
        if n == 0:
            return np.zeros((0, self.d), np.float32)
        out = self.pq.decode(self._codes[i0:i0 + n])
        if isinstance(out, np.ndarray):
            out = torch.from_numpy(out)
        lists = self._lists[i0:i0 + n]
        if self.by_residual:
            out = out + self.quantizer._c[lists.clamp(min=0)]
        out = torch.where((lists < 0)[:, None], torch.full_like(out, float("nan")), out)
        return self.backend.to_host(out.contiguous())

    def reconstruct(self, i):
        return self.reconstruct_n(i, 1)[0]


class ResidualQuantizer:
    """Residual vector quantiser (RVQ: SoundStream, EnCodec; faiss calls the family ResidualQuantizer): M codebooks of
    ksub = 256 words of d features.  Stage 0 quantises the frame, stage m what the stages before it left over; M
    one-byte tokens per frame, coarse to fine.  max_beam_size = B, 1 <= B <= 32, keeps the B best partial codes of every
    frame alive through the stages (B = 1: the greedy encoder, every prefix of a code a valid coarser code; faiss's own
    default is 5).  One plain k-means per stage; the contract below is the library's own, recalled from faiss and not
    verified against its output: faiss's look-up-table beam search, which changes the arithmetic, and its
    progressive-dimension training are not implemented.  nbits != 8 and a max_beam_size outside 1 .. 32 raise
    NotImplementedError, and so does max_beam_size > 1 on a backend that has neither rq_beam_step() nor knn().

    The beam.  After stage m a row i has B_m beams, B_0 = 1 and B_{m+1} = min(B, B_m * ksub); beam s has a residual
    R_m[i, s] (fp32), R_0[i, 0] = x[i], the codes of its path and the distance at which each ancestor was chosen.
    Stage m: (D, I) = IndexFlatL2(d) holding codebook m asked .search(R_m.reshape(n * B_m, d), k_m) with
    k_m = min(B_{m+1}, ksub), at_knn_f32's answer for that one call bit for bit (so the direct form is chosen by
    n * B_m < 20; with B = 1 this is the greedy rule).  The candidates of row i are the (s, t) with I[i * B_m + s, t] >= 0;
    the new beams are the B_{m+1} smallest by (D, s, I), lexicographic and ascending -- on equal distances the lower
    parent slot wins, then the lower word -- slot 0 the best, and R_{m+1}[i, s'] = R_m[i, s] - codebook[m, I], one fp32
    subtraction per feature.  A slot for which no candidate is left (only on rows with NaN, Inf or overflowing distances)
    follows every filled slot, takes parent slot 0, code 0 and distance +inf, subtracts word 0 from parent 0's residual,
    raises the call's flag, and is a beam like any other at the next stage.

    train(x): for m = 0 .. M-1 in order, codebook m is bit for bit the `centroids` of Kmeans(d, 256, niter=niter,
    seed=seed, max_points_per_centroid=..., backend=backend).train(R_m.reshape(n * B_m, d)) -- the residuals of all
    beams, row-major, beam-minor -- and R_{m+1} is one beam stage over ALL rows (not the subsample).  Every stage uses
    the same seed; codebook 0 is the plain Kmeans vocabulary.  Kmeans's errors and its small-training-set warning pass
    through.

    compute_codes(x) -> uint8 [n, M] (numpy for host input, a device tensor on the caller's current stream for device
    input): the path of slot 0 behind the last stage.  The call raises RuntimeError in faiss's words when the flag is up,
    unless check_finite=False, which returns the codes and skips the one host read.  return_distances=True also returns
    float32 [n, M], the distance at which that path's stage-m ancestor was chosen (column M-1 is the squared
    reconstruction error in the expansion form), return_residual=True R_M[:, 0], float32 [n, d]; the tuple is (codes,
    dist, residual).  With B = 1: r_{m+1}[i] = r_m[i] - codebook[m, codes[i, m]] and codes[i, m] is .search(r_m, 1).

    decode(codes) -> float32 [n, d]: codebook[0, codes[:, 0]] copied, then + codebook[m, codes[:, m]] for m = 1 .. M-1 in
    ascending order, one fp32 addition each.  (decode(codes) + residual is not x bit for bit: fp32 addition does not
    invert the subtractions.)

    Routes.  B = 1: a backend with rq_encode() / rq_decode() (HipBackend: csrc/rq.hip) does each call in the library, all
    M stages in one launch at d = 64 and 128; any other backend composes one assign() per stage and a torch subtraction,
    and decodes by indexing and adding.  B > 1: rq_beam_encode() (HipBackend: csrc/rq_beam.hip) does the call in the
    library; a backend with rq_beam_step() runs the stages one by one and follows the parents back in torch; a backend
    with only knn() composes each stage from knn(), a stable torch sort on D over the (s, t) candidates in row-major
    order (which is the (D, s, I) order, a list being in (D, I) order already), a gather and a subtraction."""

    def __init__(self, d, M, nbits=8, niter=25, seed=1234, max_points_per_centroid=256, max_beam_size=1, verbose=False,
                 backend=None):
        d, M, nbits, max_beam_size = int(d), int(M), int(nbits), int(max_beam_size)
        if M < 1 or d < 1:
            raise ValueError(f"ResidualQuantizer: d = {d} and M = {M} must both be at least 1")
        if nbits != 8:
            raise NotImplementedError(f"ResidualQuantizer: nbits = {nbits} (only 8-bit codes, one byte per stage, are implemented)")
        if not 1 <= max_beam_size <= 32:
            raise NotImplementedError(f"ResidualQuantizer: max_beam_size = {max_beam_size} (beams of 1 to 32 are "
                                      "implemented: the exact top-k sweep stops at 32)")
        self.d, self.M, self.nbits, self.max_beam_size = d, M, nbits, max_beam_size
        self.ksub, self.code_size = 256, M
        self.niter, self.seed, self.verbose = int(niter), int(seed), bool(verbose)
        self.max_points_per_centroid = int(max_points_per_centroid)
        self.backend = backend or default_backend()
        if max_beam_size > 1 and not (hasattr(self.backend, "rq_beam_step") or hasattr(self.backend, "knn")):
            raise NotImplementedError(f"ResidualQuantizer: max_beam_size = {max_beam_size} needs a backend with "
                                      "rq_beam_step() or knn()")
        self.centroids_device = None   # [M, ksub, d] device tensor after train() / set_centroids()
        self._centroids_host = None

    @property
    def is_trained(self) -> bool:
        return self.centroids_device is not None

    @property
    def centroids(self):
        """numpy [M, ksub, d] float32 (None before training)."""
        if self._centroids_host is None and self.centroids_device is not None:
            self._centroids_host = self.backend.to_host(self.centroids_device)
        return self._centroids_host

    def set_centroids(self, c) -> None:
        """Takes a ready [M, 256, d] table (host or device) without training."""
        c = self.backend._f32(c)
        want = (self.M, self.ksub, self.d)
        if tuple(c.shape) != want:
            raise ValueError(f"ResidualQuantizer.set_centroids: expected {list(want)}, got {list(c.shape)}")
        self.centroids_device = c.clone()
        self._centroids_host = None

    def _rows(self, x, what):
        x = self.backend._f32(x)
        assert x.dim() == 2 and x.shape[1] == self.d, f"{what}: expected [n, {self.d}], got {tuple(x.shape)}"
        return x

    def _require_trained(self, what):
        if not self.is_trained:
            raise RuntimeError(f"ResidualQuantizer.{what}: the quantiser is not trained (call train() or set_centroids())")

    def _beam_step_composed(self, r, b_in, book, b_out):
        """One beam stage from the backend's knn(): a stable sort on D over the candidates s * k + t, a gather and a
        subtraction.  Arguments and results as _beam_step."""
        d = book.shape[1]
        k = min(b_out, book.shape[0])
        ids, dis = self.backend.knn(r.reshape(-1, d), book, k)
        n = ids.shape[0] // b_in
        ids, dis = ids.view(n, b_in * k), dis.view(n, b_in * k)
        top, order = torch.sort(dis, dim=1, stable=True)      # equal distances stay in (s, I) order
        top, order = top[:, :b_out].contiguous(), order[:, :b_out]
        filled = top < float("inf")
        parent = torch.where(filled, order // k, torch.zeros_like(order))
        code = torch.where(filled, ids.gather(1, order), torch.zeros_like(order))
        rows = torch.arange(n, device=r.device).unsqueeze(1)
        r_out = r.reshape(n, b_in, d)[rows, parent] - book[code]
        bad = (~filled).any().reshape(1).to(torch.int32)
        return r_out.contiguous(), parent.to(torch.int32), code.to(torch.uint8), top, bad

    def _beam_step(self, r, b_in, book, b_out):
        """One beam stage: r [n, b_in, d] or [n * b_in, d] -> (r_out [n, b_out, d], parent int32, code uint8, dist float32
        [n, b_out], bad int32 [1]), on the backend's device."""
        if hasattr(self.backend, "rq_beam_step"):
            return self.backend.rq_beam_step(r, b_in, book, b_out)
        return self._beam_step_composed(r, b_in, book, b_out)

    def _encode_by_stages(self, x, cb, want_dist, want_residual, step=None):
        """The beam encode as one beam stage per codebook (step: _beam_step, or _beam_step_composed) and the walk back
        from slot 0 through the parents in torch."""
        step = step or self._beam_step
        B, ksub = self.max_beam_size, cb.shape[1]
        r, b = x, 1
        steps, bad = [], None
        for m in range(cb.shape[0]):
            b_out = min(B, b * ksub)
            r, parent, code, dist, bad_m = step(r, b, cb[m], b_out)
            steps.append((parent, code, dist))
            bad = bad_m if bad is None else bad | bad_m
            b = b_out
        n = x.shape[0]
        slot = torch.zeros((n, 1), dtype=torch.int64, device=x.device)
        codes, dists = [], []
        for parent, code, dist in reversed(steps):
            codes.append(code.gather(1, slot))
            dists.append(dist.gather(1, slot))
            slot = parent.gather(1, slot).to(torch.int64)
        return (torch.cat(codes[::-1], 1).contiguous(), torch.cat(dists[::-1], 1).contiguous() if want_dist else None,
                r[:, 0].contiguous() if want_residual else None, bad)

    def _encode(self, x, cb, want_dist, want_residual):
        """-> (codes, dist or None, residual or None, bad int32 [1]) on the backend's device, nothing read back."""
        be = self.backend
        if self.max_beam_size > 1:
            if hasattr(be, "rq_beam_encode"):
                return be.rq_beam_encode(x, cb, self.max_beam_size, want_dist=want_dist, want_residual=want_residual)
            return self._encode_by_stages(x, cb, want_dist, want_residual)
        if hasattr(be, "rq_encode"):
            return be.rq_encode(x, cb, want_dist=want_dist, want_residual=want_residual)
        r, ids, dis = x, [], []
        for m in range(cb.shape[0]):
            i_m, d_m = be.assign(r, cb[m], want_dist=want_dist)
            ids.append(i_m)
            if want_dist:
                dis.append(torch.where(i_m < 0, torch.full_like(d_m, float("inf")), d_m))
            if want_residual or m + 1 < cb.shape[0]:
                r = r - cb[m][i_m.clamp(min=0)]
        ids = torch.stack(ids, 1)
        bad = (ids < 0).any().reshape(1).to(torch.int32)
        return (ids.clamp(min=0).to(torch.uint8), torch.stack(dis, 1).contiguous() if want_dist else None,
                r.contiguous() if want_residual else None, bad)

    def train(self, x) -> None:
        be = self.backend
        r = self._rows(x, "ResidualQuantizer.train")
        books, b = [], 1
        for m in range(self.M):
            km = Kmeans(self.d, self.ksub, niter=self.niter, verbose=self.verbose, seed=self.seed,
                        max_points_per_centroid=self.max_points_per_centroid, backend=be)
            km.train(r.reshape(-1, self.d))
            books.append(km.centroids_device)
            if m + 1 < self.M:
                if self.max_beam_size > 1:
                    b_out = min(self.max_beam_size, b * self.ksub)
                    r, b = self._beam_step(r, b, km.centroids_device, b_out)[0], b_out
                else:
                    r = self._encode(r, km.centroids_device.unsqueeze(0), False, True)[2]
        self.centroids_device = torch.stack(books, 0).contiguous()
        self._centroids_host = None

    def compute_codes(self, x, return_distances=False, return_residual=False, check_finite=True):
        self._require_trained("compute_codes")
        be = self.backend
        host = _is_host(x)
        x = self._rows(x, "ResidualQuantizer.compute_codes")
        if x.shape[0] == 0:
            codes, bad = be.empty((0, self.M), torch.uint8), None
            dist = be.empty((0, self.M)) if return_distances else None
            res = be.empty((0, self.d)) if return_residual else None
        else:
            codes, dist, res, bad = self._encode(x, self.centroids_device, return_distances, return_residual)
        if check_finite and bad is not None and int(bad.item()):
            raise RuntimeError("Error: 'std::isfinite(x_in[i])' failed: input contains NaN's or Inf's")
        out = [codes] + ([dist] if return_distances else []) + ([res] if return_residual else [])
        if host:
            out = [be.to_host(t) for t in out]
        return out[0] if len(out) == 1 else tuple(out)

    def decode(self, codes):
        self._require_trained("decode")
        be = self.backend
        host = _is_host(codes)
        if isinstance(codes, np.ndarray):
            codes = torch.from_numpy(np.ascontiguousarray(codes))
        assert codes.dim() == 2 and codes.shape[1] == self.M and codes.dtype == torch.uint8, \
            f"ResidualQuantizer.decode: expected uint8 [n, {self.M}]"
        cb = self.centroids_device
        if hasattr(be, "rq_decode"):
            out = be.rq_decode(codes, cb)
        else:
            idx = codes.to(torch.int64)
            out = cb[0][idx[:, 0]].clone()
            for m in range(1, self.M):
                out = out + cb[m][idx[:, m]]
        return be.to_host(out) if host else out


class AudioTokenizer:
    """Audio -> token ids against a trained vocabulary, without a spectrogram leaving the device: what the reference
    does with get_spectrogram + get_sequence (tools/manual_tester.py), and what SpectrogramGenerator.run() followed by
    SpecTokenizer.run() compute through .npy files -- same tokens.

    centroids: the vocabulary, [k, d] (numpy or tensor), or an IndexFlatL2 that holds it.  d = n_mels, or
    n_mels * num_kernels with `conv`, the nn.Conv1d(1, num_kernels, kernel_size, padding) of config.use_convolution.
    normalize: config.normalize, the per-clip (spec - min) / (max - min).  One batch is one ragged front-end call
    (frame-major rows; unit rows and the scaling in the same log-mel call), the convolution and its row normalisation if
    any, one nearest-centroid search, and two device->host copies: the tokens and the per-clip flags.
    AudioTokenizer.from_features(centroids, features): an ops.MFCC instance replaces the log-mel rows by its features
    between the front-end call and the search (frontend_ragged without unit rows, HipBackend.mfcc, l2norm_rows, the
    search); the vocabulary is then [k, D] with D = features.D."""

    def __init__(self, centroids, sample_rate=22050, n_fft=512, hop_length=128, n_mels=64, normalize=False, conv=None,
                 fb=None, backend=None):
        self._setup(centroids, sample_rate, n_fft, hop_length, n_mels, normalize, conv, fb, backend, None)

    @classmethod
    def from_features(cls, centroids, features, normalize=False, conv=None, fb=None, backend=None):
        """The tokenizer of a vocabulary trained on `features` (an ops.MFCC instance): sample rate, transform size, hop
        and n_mels of the front end are the instance's own, and so are fb and the backend unless given.  (A constructor
        of its own rather than one more keyword: tests/test_audio_tokens_abi.py pins the argument list of __init__.)  conv has
        no meaning here and raises ValueError."""
        if conv is not None:
            raise ValueError("AudioTokenizer: features and conv cannot be combined")
        if not isinstance(features, MFCC):
            raise ValueError("AudioTokenizer: features must be an ops.MFCC instance")
        self = cls.__new__(cls)
        self._setup(centroids, features.sample_rate, features.n_fft, features.hop_length, features.n_mels, normalize, None,
                    features.fb if fb is None else fb, backend or features.backend, features)
        return self

    def _setup(self, centroids, sample_rate, n_fft, hop_length, n_mels, normalize, conv, fb, backend, features):
        self.features = features
        self.backend = be = backend or default_backend()
        if isinstance(centroids, IndexFlatL2):
            self.index = centroids
        else:
            c = be._f32(centroids)
            self.index = IndexFlatL2(c.shape[1], backend=be)
            self.index.add(c)
        self.sample_rate, self.n_fft, self.hop_length, self.n_mels = sample_rate, n_fft, hop_length, n_mels
        self.normalize, self.conv = bool(normalize), conv
        self.fb = None if fb is None else be._f32(fb)
        d = n_mels * (conv.weight.shape[0] if conv is not None else 1) if features is None else features.D
        assert self.index.d == d, f"centroids are [k, {self.index.d}], the frames [n, {d}]"
        self.last_tokens = None   # device int64: the tokens of the last batch's kept clips, clip after clip

    def encode(self, waveforms, sample_rates=None):
        """-> one entry per clip, in input order: its tokens, a host int64 tensor [T_i], or None where the reference
        would skip the clip (too short for the reflect padding; a NaN or Inf in its spectrogram -- under normalize, a
        constant clip too).  waveforms: what HipBackend.frontend_ragged takes -- [C_i, L_i] or [L_i] tensors on either
        side, or (flat, table) as the FLAC decoder leaves it; sample_rates: one per clip, or one for all (default:
        self.sample_rate)."""
        be = self.backend
        n = len(waveforms[1]) if isinstance(waveforms, tuple) else len(waveforms)
        self.last_tokens = None
        if n == 0:
            return []
        rates = self.sample_rate if sample_rates is None else sample_rates
        rows, T, first, bad = be.frontend_ragged(waveforms, rates, self.sample_rate, self.n_fft, self.hop_length, self.n_mels,
                                                 fb=self.fb, frame_major=True,
                                                 l2norm=self.conv is None and self.features is None,
                                                 minmax=self.normalize)
        if rows.shape[0] == 0:
            return [None] * n
        if self.features is not None:
            rows = be.l2norm_rows(self.features.of_rows(rows, T))
        if self.conv is not None:
            with torch.no_grad():
                bias = self.conv.bias.detach() if self.conv.bias is not None else None
                rows = be.l2norm_rows(be.conv1d_mel(rows, self.conv.weight.detach(), bias, padding=int(self.conv.padding[0])))
        tokens_dev, _ = self.index.assign(rows, want_dist=False)
        tokens, bad = torch.from_numpy(be.to_host(tokens_dev)), be.to_host(bad)
        keep = (T > 0) & (bad == 0)
        # (the rows of a flagged clip hold NaN and their tokens mean nothing: dropped here, and from last_tokens)
        self.last_tokens = tokens_dev if not bad.any() else tokens_dev[be.from_host(np.repeat(keep, T))]
        return [tokens[int(first[i]): int(first[i]) + int(T[i])] if keep[i] else None for i in range(n)]

    def encode_files(self, paths):
        """encode() for audio files: the batch's .flac files in one device decode, other formats on the host, as
        SpectrogramGenerator reads them.  None for a file that does not decode, too."""
        import logging

        from .processors.spectrogram_generator import decode_batch
        got = decode_batch(paths, self.backend, logging.getLogger(__name__))
        live = [i for i, g in enumerate(got) if g is not None]
        tokens = self.encode([got[i][0] for i in live], [got[i][1] for i in live])
        out = [None] * len(got)
        for i, t in zip(live, tokens):
            out[i] = t
        return out


def _check_random_state(seed):
    """sklearn.utils.check_random_state: None -> numpy's global RandomState, an int -> a new RandomState(seed), a
    RandomState -> itself."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError("%r cannot be used to seed a numpy.random.RandomState instance" % seed)


def _labels_int64(labels):
    """Integer labels as they are (only the distinct values matter); any other kind through np.unique, as sklearn's
    LabelEncoder."""
    if isinstance(labels, torch.Tensor):
        if labels.dtype.is_floating_point or labels.dtype.is_complex:
            labels = labels.cpu().numpy()
        else:
            return labels.reshape(-1).to(torch.int64)
    labels = np.asarray(labels).reshape(-1)
    if labels.dtype.kind not in "iub":
        labels = np.unique(labels, return_inverse=True)[1].reshape(-1)
    return torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64))


def silhouette_samples(X, labels, backend=None):
    """sklearn.metrics.silhouette_samples(X, labels) (euclidean) on the device: numpy float32 [n], exact.

    X: numpy array or torch tensor [n, d], on the host or the device; other float dtypes are converted to float32 first
    and the result is sklearn's float32 computation on those rows.  labels: [n] of any values.  The recipe and its
    rounding points are at_silhouette_f32's (include/audio_tokens_amd.h)."""
    be = backend or default_backend()
    return be.to_host(be.silhouette_samples(X, _labels_int64(labels)))


def silhouette_score(X, labels, *, sample_size=None, random_state=None, backend=None):
    """sklearn.metrics.silhouette_score(X, labels, sample_size=..., random_state=...) (euclidean) on the device: the
    mean silhouette as a Python float (fp64 sum of the fp32 samples / n).

    The sample is sklearn's own draw, made on the host: check_random_state(random_state).permutation(n)[:sample_size]
    (None: numpy's global RandomState, which advances exactly as under sklearn); the sampled rows are gathered on the
    device.  X as for silhouette_samples (other float dtypes become float32)."""
    be = backend or default_backend()
    labels = _labels_int64(labels)
    if sample_size is not None:
        x = be._f32(X)
        n = x.shape[0]
        if labels.numel() != n:
            raise ValueError(f"Found input variables with inconsistent numbers of samples: [{n}, {labels.numel()}]")
        if be.any_nonfinite(x):
            raise ValueError("Input X contains NaN or infinity.")
        idx = _check_random_state(random_state).permutation(n)[:sample_size]
        X = be.gather_rows(x, idx.astype(np.int32))
        labels = labels.to(be.device)[be.from_host(idx.astype(np.int64))]
    total = be.empty((1,), torch.float64)
    s = be.silhouette_samples(X, labels, sum_out=total)
    return float(total.item()) / s.numel()


def _raise_for_flags(flags):
    """The flag word of the metric kernels (bit 0 a non-finite score, bit 1 a label other than 0 / 1) as ValueError."""
    if flags & 1:
        raise ValueError("Input y_score contains NaN or infinity.")
    if flags & 2:
        raise ValueError("Labels must be 0 or 1 in every class (multilabel-indicator format): found another value.")


def _average_precision_checked(labels, scores, be):
    """be.average_precision and the one host read behind it: (ap, n_pos) device tensors, map_pair as two floats."""
    ap, n_pos, pair = be.average_precision(scores, labels)
    tail = torch.cat([pair, be.ap_flags.double()]).cpu()        # the only synchronisation
    _raise_for_flags(int(tail[2]))
    return ap, n_pos, float(tail[0]), float(tail[1])


def average_precision(labels, scores, backend=None):
    """sklearn.metrics.average_precision_score(labels[:, j], scores[:, j]) for every class j on the device: numpy
    float64 [c], NaN for the classes without a positive (the classes the reference skips).

    labels, scores: [n, c] numpy arrays or torch tensors, on the host or the device; scores of other float dtypes and
    bool / integer labels become float32 on the device.  Raises ValueError for NaN / infinite scores, as sklearn, and
    for labels other than 0 and 1.  The recipe and its error bound are at_average_precision_f32's
    (include/audio_tokens_amd.h)."""
    be = backend or default_backend()
    ap, _, _, _ = _average_precision_checked(labels, scores, be)
    return be.to_host(ap)


def mean_average_precision(labels, scores, backend=None):
    """The reference's MetricsCalculator.calculate_mAP(labels, predictions): the mean of the per-class average precision
    over the classes with at least one positive, 0.0 when there is none; a Python float.  Inputs and errors as for
    average_precision; one host read (flags and the sum) at the end is the only synchronisation."""
    be = backend or default_backend()
    _, _, total, count = _average_precision_checked(labels, scores, be)
    return total / count if count > 0 else 0.0


def _roc_auc_checked(labels, scores, be):
    """be.ranking_metrics without the average precision and the one host read behind it: auc as a device tensor, the
    mAUC pair as two floats."""
    out = be.ranking_metrics(scores, labels, want_ap=False)
    tail = torch.cat([out["mauc"], be.ap_flags.double()]).cpu()  # the only synchronisation
    _raise_for_flags(int(tail[2]))
    return out["auc"], float(tail[0]), float(tail[1])


def roc_auc(labels, scores, backend=None):
    """sklearn.metrics.roc_auc_score(labels[:, j], scores[:, j]) for every class j on the device, in exact arithmetic
    (at_ranking_metrics_f32): numpy float64 [c], NaN for the classes without a positive or without a negative (where
    sklearn raises).  Inputs and errors as for average_precision."""
    be = backend or default_backend()
    auc, _, _ = _roc_auc_checked(labels, scores, be)
    return be.to_host(auc)


def mean_roc_auc(labels, scores, backend=None):
    """mAUC, the AudioSet convention and the counterpart of mean_average_precision's rule: the mean of the per-class ROC
    AUC over the classes with both a positive and a negative, 0.0 when there is none; a Python float."""
    be = backend or default_backend()
    _, total, count = _roc_auc_checked(labels, scores, be)
    return total / count if count > 0 else 0.0


def roc_auc_score(y_true, y_score, backend=None):
    """sklearn.metrics.roc_auc_score for one binary problem: y_true, y_score 1-D; raises sklearn's ValueError when only
    one class is present."""
    be = backend or default_backend()
    y, s = (torch.as_tensor(a) if not isinstance(a, np.ndarray) else torch.from_numpy(np.ascontiguousarray(a))
            for a in (y_true, y_score))
    if y.dim() != 1 or s.dim() != 1:
        raise ValueError(f"roc_auc_score takes 1-D input: got {tuple(y.shape)}, {tuple(s.shape)}")
    _, total, count = _roc_auc_checked(y.reshape(-1, 1), s.reshape(-1, 1), be)
    if count == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return total


def d_prime(auc):
    """The sensitivity index AudioSet results carry beside mAP and mAUC: sqrt(2) * Phi^-1(auc), on the host from the
    standard library; +inf / -inf at 1 / 0, NaN for NaN."""
    auc = float(auc)
    if math.isnan(auc):
        return float("nan")
    if auc <= 0.0 or auc >= 1.0:
        return math.copysign(float("inf"), auc - 0.5)
    return math.sqrt(2.0) * statistics.NormalDist().inv_cdf(auc)


def _f1_and_hamming(counts, n):
    """counts: [c][3] Python ints (tp, fp, fn) -> (per-class F1 list, micro, macro, Hamming loss), sklearn's multilabel
    rules with zero_division=0.  Every ratio is one correctly rounded fp64 division of exact integers; the macro mean is
    the correctly rounded sum of the per-class ratios over c."""
    per_class = [2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0 for tp, fp, fn in counts]
    tp, fp, fn = (sum(col) for col in zip(*counts))
    micro = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
    return per_class, micro, math.fsum(per_class) / len(counts), (fp + fn) / (n * len(counts))


def _threshold_counts_checked(labels, scores, threshold, be):
    """be.threshold_counts and the one host read behind it: ([c][3] Python ints, n)."""
    counts = be.threshold_counts(scores, labels, threshold)
    host = torch.cat([counts.reshape(-1), be.tc_flags.to(torch.int64)]).cpu().tolist()   # the only synchronisation
    _raise_for_flags(host[-1])
    return [host[i:i + 3] for i in range(0, len(host) - 1, 3)], len(labels)


def f1_score(labels, scores, threshold, average="macro", backend=None):
    """sklearn.metrics.f1_score(labels, scores > threshold, average=average, zero_division=0) for multilabel input, the
    counting on the device (at_threshold_counts_f32; the comparison is numpy's: strict, in float32).  "macro": the mean
    over all c classes, a class without positives and predictions counting 0; "micro": from the summed counts; None:
    numpy float64 [c].  Unlike sklearn's thresholding, which would quietly take NaN as not predicted, non-finite scores
    raise ValueError, as do labels other than 0 and 1."""
    if average not in ("macro", "micro", None):
        raise ValueError(f"average has to be 'macro', 'micro' or None: got {average!r}")
    counts, n = _threshold_counts_checked(labels, scores, threshold, backend or default_backend())
    per_class, micro, macro, _ = _f1_and_hamming(counts, n)
    return np.asarray(per_class, np.float64) if average is None else micro if average == "micro" else macro


def hamming_loss(labels, scores, threshold, backend=None):
    """sklearn.metrics.hamming_loss(labels, scores > threshold) for multilabel input: (fp + fn) / (n c).  Counting and
    errors as for f1_score."""
    counts, n = _threshold_counts_checked(labels, scores, threshold, backend or default_backend())
    return _f1_and_hamming(counts, n)[3]


def classification_metrics(labels, scores, threshold=0.2, backend=None):
    """What the reference's trainer logs after an epoch (utils/metrics_calculator.py:8-33, the threshold metrics it
    comments out included) and the AudioSet triple: {"mAP", "mAUC", "d_prime", "f1_score_micro", "f1_score_macro",
    "hamming_loss"} as Python floats.  One ranking_metrics call (one sort per class chunk), one threshold_counts call
    and one device-to-host read; d_prime = d_prime(mAUC)."""
    be = backend or default_backend()
    rank = be.ranking_metrics(scores, labels)
    counts = be.threshold_counts(scores, labels, threshold)
    host = torch.cat([counts.reshape(-1), rank["map"].view(torch.int64), rank["mauc"].view(torch.int64),
                      be.ap_flags.to(torch.int64), be.tc_flags.to(torch.int64)]).cpu()   # the only synchronisation
    _raise_for_flags(int(host[-1]) | int(host[-2]))
    map_sum, map_count, auc_sum, auc_count = host[-6:-2].view(torch.float64).tolist()
    flat = host[:-6].tolist()
    _, micro, macro, hamming = _f1_and_hamming([flat[i:i + 3] for i in range(0, len(flat), 3)], len(labels))
    mauc = auc_sum / auc_count if auc_count > 0 else 0.0
    return {"mAP": map_sum / map_count if map_count > 0 else 0.0, "mAUC": mauc, "d_prime": d_prime(mauc),
            "f1_score_micro": micro, "f1_score_macro": macro, "hamming_loss": hamming}
