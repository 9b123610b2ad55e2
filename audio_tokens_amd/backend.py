"""Tensor-level front end of the C ABI: PyTorch-ROCm tensors in, PyTorch-ROCm tensors out.

`HipBackend` is the only compute backend the package ships.  It hands `data_ptr()`s and the
current HIP stream to libaudio_tokens_amd.so and never computes anything itself; if the library
or a gfx950 device is missing it raises.  (tests/ drive the same host logic with a CPU stand-in
built on the oracle, to cover the multi-rank code path under gloo; that stand-in lives in tests/,
not here.)
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib

_vp = ctypes.c_void_p


def _ptr(t) -> _vp:
    return _vp(t.data_ptr()) if t is not None else _vp(None)


def _np_ptr(a: np.ndarray) -> _vp:
    return _vp(a.ctypes.data)


class HostHelpers:
    """The sequential, RNG-driven host pieces of the FAISS recipe (native C++, no GPU needed)."""

    def __init__(self):
        self.lib = _lib.load()
        self._groupings = {}   # fingerprint of a centroid table -> device grouping (remember_grouping)

    def rand_perm(self, n: int, seed: int) -> np.ndarray:
        out = np.empty(n, np.int32)
        _lib.check(self.lib.at_rand_perm_mt19937(n, seed, _np_ptr(out)))
        return out

    def rand_perm_prefix(self, n: int, seed: int, m: int) -> np.ndarray:
        out = np.empty(m, np.int32)
        _lib.check(self.lib.at_rand_perm_prefix_mt19937(n, seed, m, _np_ptr(out)))
        return out

    def mel_filterbank(self, sample_rate: int, n_fft: int, n_mels: int) -> np.ndarray:
        fb = np.empty((n_fft // 2 + 1, n_mels), np.float32)
        _lib.check(self.lib.at_mel_filterbank_host(sample_rate, n_fft, n_mels, _np_ptr(fb)))
        return fb

    def num_frames(self, L: int, hop: int) -> int:
        return int(self.lib.at_num_frames(L, hop))

    def group_rows_kd(self, rows: np.ndarray, leaf: int = 32) -> np.ndarray:
        """Spatial grouping of a host table into groups of `leaf` rows (-1 padded permutation).  A permutation whatever
        the table holds (NaN, +-inf, any magnitude); a table scaled by a power of two inside the normal range gets the
        same cuts."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        k, d = rows.shape
        out = np.empty(((k + leaf - 1) // leaf) * leaf, np.int32)
        _lib.check(self.lib.at_group_rows_kd_host(_np_ptr(rows), k, d, leaf, _np_ptr(out)))
        return out

    # The grouping never decides a result, so a weak fingerprint of the table is enough to hand the grouping
    # a Kmeans ended with to the IndexFlatL2 later built from the same centroids (a mismatch costs speed only).
    @staticmethod
    def _table_fingerprint(rows: np.ndarray):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        return rows.shape, int(rows.view(np.uint32).sum(dtype=np.uint64))

    def remember_grouping(self, rows: np.ndarray, cperm) -> None:
        cache = self._groupings
        if len(cache) >= 4:
            cache.pop(next(iter(cache)))
        cache[self._table_fingerprint(rows)] = cperm

    def recall_grouping(self, rows: np.ndarray):
        return self._groupings.get(self._table_fingerprint(rows))

    def resample_taps(self, orig_freq: int, new_freq: int):
        """-> (taps float32 [new, 2*width + orig], orig, new, width): torchaudio's sinc_interp_hann kernel."""
        o, nw, w = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(self.lib.at_resample_taps_host(orig_freq, new_freq, ctypes.byref(o), ctypes.byref(nw),
                                                  ctypes.byref(w), None, 0))
        taps = np.empty((nw.value, 2 * w.value + o.value), np.float32)
        _lib.check(self.lib.at_resample_taps_host(orig_freq, new_freq, ctypes.byref(o), ctypes.byref(nw),
                                                  ctypes.byref(w), _np_ptr(taps), taps.size))
        return taps, o.value, nw.value, w.value

    def resample_length(self, L: int, orig_freq: int, new_freq: int) -> int:
        return int(self.lib.at_resample_length(L, orig_freq, new_freq))

    def flac_index(self, data: bytes):
        """One FLAC file's bytes -> (facts, frames): facts = {"channels", "bits_per_sample", "sample_rate",
        "total_samples", "min_block", "max_block", "variable_blocksize"}, frames = numpy records
        (_lib.FLAC_FRAME_FIELDS: offset, length, first_sample, block_size, channel_assignment, bits_per_sample, ...), one
        per audio frame, none decoded.  Raises NativeError with code AT_E_FLAC_NOT_FLAC / _UNSUPPORTED / _CORRUPT."""
        buf = np.frombuffer(data, dtype=np.uint8)
        info, n = _lib.FlacInfo(), ctypes.c_int64(0)
        cap = max(64, buf.size // 512)
        while True:
            frames = np.zeros(cap, dtype=np.dtype(_lib.FLAC_FRAME_FIELDS))
            _lib.check(self.lib.at_flac_index_host(_np_ptr(buf) if buf.size else _np_ptr(np.zeros(1, np.uint8)), buf.size,
                                                   ctypes.byref(info), _np_ptr(frames), cap, ctypes.byref(n)))
            if n.value <= cap:
                break
            cap = int(n.value)
        facts = {name: int(getattr(info, name)) for name, _ in _lib.FlacInfo._fields_}
        return facts, frames[:n.value]

    def frontend_plan(self, channels, lengths, rates, common_sr, n_fft, hop, offsets=None, row_strides=None):
        """at_frontend_plan_host: the layout of a batch of clips of unequal length, channel count (1 or 2) and sample
        rate -> (plan, order, groups, totals): numpy records per clip (_lib.FRONTEND_CLIP_FIELDS), the clip indices
        sorted by group, one record per reduced rate pair (_lib.FRONTEND_GROUP_FIELDS) and the int64 totals as a dict.
        offsets / row_strides (floats) say where every clip's [C, L] block lies in the input buffer; by default the
        blocks lie back to back."""
        n = len(lengths)
        cin = np.zeros(n, np.dtype(_lib.FRONTEND_CLIP_IN_FIELDS))
        cin["channels"], cin["length"], cin["rate"] = channels, lengths, rates
        cin["row_stride"] = cin["length"] if row_strides is None else row_strides
        if offsets is None:
            sizes = cin["channels"].astype(np.int64) * cin["length"]
            cin["offset"] = np.cumsum(sizes) - sizes
        else:
            cin["offset"] = offsets
        plan = np.zeros(n, np.dtype(_lib.FRONTEND_CLIP_FIELDS))
        order = np.zeros(n, np.int32)
        cap = 16
        while True:
            groups = np.zeros(cap, np.dtype(_lib.FRONTEND_GROUP_FIELDS))
            totals = np.zeros(1, np.dtype(_lib.FRONTEND_TOTALS_FIELDS))
            try:
                _lib.check(self.lib.at_frontend_plan_host(_np_ptr(cin), n, common_sr, n_fft, hop, _np_ptr(plan),
                                                          _np_ptr(order), _np_ptr(groups), cap, _np_ptr(totals)))
                break
            except _lib.NativeError as e:
                if "rate pairs" not in str(e) or cap >= max(n, 16):
                    raise
                cap = max(n, 16)
        tot = {name: int(totals[0][name]) for name, _ in _lib.FRONTEND_TOTALS_FIELDS}
        return plan, order, groups[:tot["n_groups"]], tot

    def dct_matrix(self, n_mfcc: int, n_mels: int, norm="ortho") -> np.ndarray:
        """at_dct_matrix_host: the DCT-II table [n_mels, n_mfcc] of ops.MFCC, cos(pi / n_mels * (n + 0.5) * k) in double,
        scaled (norm "ortho": column 0 by 1/sqrt(2), then all by sqrt(2 / n_mels); None: all by 2), rounded to float32
        once."""
        if norm not in ("ortho", None):
            raise ValueError('norm must be "ortho" or None')
        out = np.empty((n_mels, n_mfcc), np.float32)
        _lib.check(self.lib.at_dct_matrix_host(n_mfcc, n_mels, 1 if norm == "ortho" else 0, _np_ptr(out)))
        return out

    @staticmethod
    def part_layout(k, d):
        """Packed per-rank partial of one Lloyd iteration, in floats: sums [k*d], counts [k], padding to an even
        offset, then the rank's objective as one double -> (offset of the double, total length)."""
        p = k * d + k
        off = p + (p & 1)
        return off, off + 2

    def split_clusters(self, hassign: np.ndarray, centroids: np.ndarray, n: int) -> int:
        """In place on two C-contiguous float32 host arrays; returns nsplit."""
        assert hassign.dtype == np.float32 and centroids.dtype == np.float32
        assert hassign.flags.c_contiguous and centroids.flags.c_contiguous
        k, d = centroids.shape
        ns = ctypes.c_int(0)
        _lib.check(self.lib.at_split_clusters_host(d, k, n, _np_ptr(hassign), _np_ptr(centroids),
                                                   ctypes.byref(ns)))
        return int(ns.value)

    # What a backend may fuse, composed from what every backend has.
    def lloyd_stats_split(self, hassign, cent, n: int, nsplit_out, parts, stats_row, objs=None) -> None:
        """lloyd_stats followed by split_clusters_device."""
        k, d = cent.shape
        self.lloyd_stats(hassign, parts, k, d, stats_row, objs=objs)
        self.split_clusters_device(hassign, cent, n, nsplit_out)

    def from_host_async(self, a, dtype=None):
        """from_host that need not drain the stream first."""
        return self.from_host(a, dtype)


class HipBackend(HostHelpers):
    def __init__(self, device=None):
        super().__init__()
        if not torch.cuda.is_available():
            raise RuntimeError("audio_tokens_amd: no ROCm device visible (torch.cuda.is_available() "
                               "is False) and there is no CPU fallback")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"audio_tokens_amd: device must be a ROCm GPU, got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.ctx = _lib.context(device.index)
        self.assign_trace = None  # set to a list to collect (kind, n, d, k, start_event, end_event)
        self.assign_trace_only = None   # a set of kinds: only those are traced (every traced launch is two events on the stream)
        # host-side A/B switches, read from the environment once (the native ones: at_debug.h, self.debug_set)
        self.frontend_calls = 0   # native calls of the ragged front end so far (frontend_ragged)
        self.frontend_bytes = 0   # bytes it uploaded
        self.switches = {"filter": os.environ.get("AT_FILTER", "1") != "0",
                         "c2f_fused": os.environ.get("AT_C2F_FUSED", "1") != "0"}

    # -- development switches (include/at_debug.h) ------------------------------------------
    def debug_set(self, name: str, value: int) -> None:
        _lib.check(self.lib.at_debug_set(self.ctx.handle, name.encode(), int(value)))

    def debug_get(self, name: str) -> int:
        v = ctypes.c_int(0)
        _lib.check(self.lib.at_debug_get(self.ctx.handle, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def diag_errors(self, reset=False) -> dict:
        """What the library met and did not treat as its own failure (include/at_debug.h: at_diag_errors): HIP errors
        found pending in the calling thread in front of one of its launches, and failures it tolerates by design."""
        stale, tol = ctypes.c_int64(0), ctypes.c_int64(0)
        sc, tc = ctypes.c_int(0), ctypes.c_int(0)
        where = ctypes.create_string_buffer(512)
        _lib.check(self.lib.at_diag_errors(ctypes.byref(stale), ctypes.byref(sc), ctypes.byref(tol), ctypes.byref(tc),
                                           where, 512, 1 if reset else 0))
        return {"stale_seen": int(stale.value), "stale_last_code": int(sc.value), "tolerated": int(tol.value),
                "tolerated_last_code": int(tc.value), "where": where.value.decode()}

    # -- plumbing --------------------------------------------------------------------------
    def _stream(self) -> _vp:
        return _vp(torch.cuda.current_stream(self.device).cuda_stream)

    def _f32(self, t, name="tensor") -> torch.Tensor:
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
        if t.dtype != torch.float32:
            t = t.float()
        if t.device != self.device:
            # (asynchronous only from pinned memory: a pageable source -- often a temporary made two lines up -- must have
            # been read by the time this returns, and torch does not wait for a non_blocking copy of one)
            t = t.to(self.device, non_blocking=t.is_pinned() if t.device.type == "cpu" else True)
        if not t.is_contiguous():
            t = t.contiguous()
        return t

    def _trace_list(self, kind):
        if self.assign_trace is None or (self.assign_trace_only is not None and kind not in self.assign_trace_only):
            return None
        return self.assign_trace

    def empty(self, shape, dtype=torch.float32) -> torch.Tensor:
        return torch.empty(shape, dtype=dtype, device=self.device)

    def zeros(self, shape, dtype=torch.float32) -> torch.Tensor:
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def from_host(self, a, dtype=None) -> torch.Tensor:
        t = torch.from_numpy(np.ascontiguousarray(a))
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.device, non_blocking=False)

    def from_host_async(self, a, dtype=None) -> torch.Tensor:
        """from_host through a pinned staging buffer: the copy is queued on the current stream and the caller goes
        on (a pageable copy would first wait for everything queued before it).  For small tables."""
        t = torch.from_numpy(np.ascontiguousarray(a))
        if dtype is not None:
            t = t.to(dtype)
        key = ("h2d", tuple(t.shape), t.dtype)
        pool = self.__dict__.setdefault("_pinned_pool", {})
        slot = pool.get(key)
        if slot is None:
            slot = pool[key] = [[torch.empty(t.shape, dtype=t.dtype).pin_memory() for _ in range(4)], 0, [None] * 4]
        i = slot[1] % 4
        if slot[2][i] is not None:
            slot[2][i].synchronize()          # (the copy that last used this staging buffer, four uploads ago)
        h = slot[0][i]
        slot[1] += 1
        h.copy_(t)
        out = h.to(self.device, non_blocking=True)
        slot[2][i] = self.record_event()
        return out

    def to_host(self, t: torch.Tensor) -> np.ndarray:
        return t.detach().cpu().numpy()

    def host_staging(self, shape, dtype) -> torch.Tensor:
        """Pinned host buffer for small asynchronous read-backs."""
        return torch.empty(shape, dtype=dtype).pin_memory()

    def synchronize(self) -> None:
        torch.cuda.current_stream(self.device).synchronize()

    def background_stream(self):
        """The context's lowest-priority stream as a torch stream (at_background_stream): `with torch.cuda.stream(s)`
        routes this backend's launches there."""
        if getattr(self, "_bg_stream", None) is None:
            h = ctypes.c_void_p()
            _lib.check(self.lib.at_background_stream(self.ctx.handle, ctypes.byref(h)))
            self._bg_stream = torch.cuda.ExternalStream(h.value, device=self.device)
        return self._bg_stream

    def record_event_timed(self):
        """record_event with timing: `a.elapsed_time(b)` between two of them once both have completed."""
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream(self.device))
        return ev

    def record_event(self):
        """Event on the current stream; `.synchronize()` on it waits for the work queued so far only."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return ev

    # -- operators ---------------------------------------------------------------------------
    def _logmel_args(self, wave, n_fft, hop, n_mels, fb):
        """What logmel and logmel_minmax share -> (wave [n_clips, L] on the device, n_clips, L, T, fb on the device)."""
        wave = self._f32(wave)
        if wave.dim() == 1:
            wave = wave.unsqueeze(0)
        assert wave.dim() == 2
        n_clips, L = wave.shape
        fbt = self._f32(fb) if fb is not None else None
        if fbt is not None:
            assert tuple(fbt.shape) == (n_fft // 2 + 1, n_mels), "fb must be [n_fft/2+1, n_mels]"
        return wave, n_clips, L, self.num_frames(L, hop), fbt

    def logmel(self, wave, sample_rate=22050, n_fft=512, hop=128, n_mels=64, fb=None,
               frame_major=False, l2norm=False, out=None) -> torch.Tensor:
        """wave [n_clips, L] (or [L]) -> [n_clips, n_mels, T], or [n_clips*T, n_mels] if frame_major.
        n_fft: any even size from 64 to 4096 (odd sizes raise NativeError: torch counts their frames differently);
        1 <= hop <= n_fft, L > n_fft/2."""
        wave, n_clips, L, T, fbt = self._logmel_args(wave, n_fft, hop, n_mels, fb)
        shape = (n_clips * T, n_mels) if frame_major else (n_clips, n_mels, T)
        if out is None:
            out = self.empty(shape)
        else:
            assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n_clips * T * n_mels
        rec = self._trace_list("logmel")
        if rec is not None:  # bench.py: HIP events on the launch stream around the launch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(self.device))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_logmel_f32(
                self.ctx.handle, _ptr(wave), n_clips, L, wave.stride(0), sample_rate, n_fft, hop, n_mels,
                _ptr(fbt), _ptr(out), _lib.AT_LAYOUT_FRAME_MAJOR if frame_major else _lib.AT_LAYOUT_MEL_MAJOR,
                1 if l2norm else 0, self._stream()))
        if rec is not None:
            e1.record(torch.cuda.current_stream(self.device))
            rec.append(("logmel", n_clips * T, n_mels, hop, e0, e1))
        return out

    def logmel_minmax(self, wave, sample_rate=22050, n_fft=512, hop=128, n_mels=64, fb=None) -> torch.Tensor:
        """wave [n_clips, L] -> [n_clips, n_mels, T]: logmel() followed by minmax_scale_clips(), one call; the extremes are
        collected by the log-mel kernel (at_logmel_minmax_f32), so the scaling is a single pass."""
        wave, n_clips, L, T, fbt = self._logmel_args(wave, n_fft, hop, n_mels, fb)
        out = self.empty((n_clips, n_mels, T))
        with torch.cuda.device(self.device):
            for c0 in range(0, n_clips, 65535):
                c1 = min(n_clips, c0 + 65535)
                _lib.check(self.lib.at_logmel_minmax_f32(
                    self.ctx.handle, _ptr(wave[c0:c1]), c1 - c0, L, wave.stride(0), sample_rate, n_fft, hop, n_mels,
                    _ptr(fbt), _ptr(out[c0:c1]), _lib.AT_LAYOUT_MEL_MAJOR, self._stream()))
        return out

    def resample(self, wave, orig_freq: int, new_freq: int) -> torch.Tensor:
        """wave [n_clips, L] (or [L]) -> [n_clips, ceil(L*new/orig)] (torchaudio Resample defaults)."""
        wave = self._f32(wave)
        squeeze = wave.dim() == 1
        if squeeze:
            wave = wave.unsqueeze(0)
        n_clips, L = wave.shape
        out_len = self.resample_length(L, orig_freq, new_freq)
        out = self.empty((n_clips, out_len))
        with torch.cuda.device(self.device):
            for c0 in range(0, n_clips, 65535):
                c1 = min(n_clips, c0 + 65535)
                _lib.check(self.lib.at_resample_f32(self.ctx.handle, _ptr(wave[c0:c1]), c1 - c0, L, wave.stride(0),
                                                    orig_freq, new_freq, _ptr(out[c0:c1]), out.stride(0), self._stream()))
        return out[0] if squeeze else out

    def frontend_ragged(self, clips, rates, common_sr, n_fft, hop, n_mels, fb=None, frame_major=False, l2norm=False,
                        pad_value=None, minmax=False):
        """Mono mix, resampler and log-mel for a batch of clips of any length, channel count and sample rate: one
        native call per rate pair present and one log-mel call, whatever the lengths (at_mix_resample_ragged_f32,
        at_logmel_ragged_f32).  Same bits as torch.mean, resample() and logmel() on each clip alone.

        clips: a list of [C, L] or [L] tensors (device tensors are read where they lie; host tensors are uploaded in
        one copy; more than two channels are mixed by torch.mean first), or what flac_decode left in self.flac_flat:
        (flat device buffer, [(offset, C, L), ...]).  rates: one rate or one per clip.
        -> (out, n_frames, first_frame, bad): out is flat, clip i's [n_mels, T_i] block at n_mels * first_frame[i]
        (frame_major: [sum T_i, n_mels], rows first_frame[i] .. + T_i); n_frames (int32) and first_frame (int64) are
        numpy arrays, T_i = 0 for a clip too short for the reflect padding (resampled length <= n_fft / 2); bad is a
        device int32 [n_clips], non-zero where the clip's output holds a NaN or Inf.  pad_value (tests): what the
        intermediate buffer's padding between clips is filled with.
        minmax: every clip's spectrogram becomes (spec - min) / (max - min), SpectrogramGenerator.normalize_spectrogram's
        bits, before the unit rows if any (at_logmel_ragged_minmax_f32: still one log-mel call); bad is then set from
        the scaled values, so a constant clip (0 / 0) is flagged too."""
        if isinstance(clips, tuple):
            flat, table = clips
            clips = [flat[o:o + C * L].view(C, L) for o, C, L in table]
        n = len(clips)
        rates = [int(rates)] * n if np.isscalar(rates) else [int(r) for r in rates]
        assert len(rates) == n, "one sample rate per clip"
        fbt = self._f32(fb) if fb is not None else None
        if fbt is not None:
            assert tuple(fbt.shape) == (n_fft // 2 + 1, n_mels), "fb must be [n_fft/2+1, n_mels]"
        blocks, host, host_floats = [], [], 0
        for w in clips:
            if isinstance(w, np.ndarray):
                w = torch.from_numpy(w)
            if w.dim() == 1:
                w = w.unsqueeze(0)
            assert w.dim() == 2, "a clip is [C, L] or [L]"
            if w.dtype != torch.float32:
                w = w.float()
            if w.shape[0] > 2:    # torch's own rounding for surround
                w = torch.mean(w, dim=0, keepdim=True)
            if w.device.type == "cpu":
                w = w.contiguous()
                host.append(w.reshape(-1))
                blocks.append((None, host_floats, w.shape[0], w.shape[1], w.shape[1]))
                host_floats += w.numel()
                continue
            if w.device != self.device:
                w = w.to(self.device)
            if w.shape[1] > 1 and w.stride(1) != 1 or w.shape[0] == 2 and w.stride(0) < w.shape[1]:
                w = w.contiguous()
            blocks.append((w, 0, w.shape[0], w.shape[1], w.stride(0) if w.shape[0] == 2 else w.shape[1]))
        up = None
        if host_floats:
            up = torch.cat(host).to(self.device)       # the batch's host clips in one copy
            self.frontend_bytes += host_floats * 4
        ptrs = [(up.data_ptr() + 4 * off) if w is None else w.data_ptr() for w, off, C, L, rs in blocks]
        live = [q for q, b in zip(ptrs, blocks) if b[3] > 0]
        base = min(live) if live else 0
        assert all((q - base) % 4 == 0 for q in live)
        offsets = [(q - base) // 4 if b[3] > 0 else 0 for q, b in zip(ptrs, blocks)]
        plan, order, groups, tot = self.frontend_plan([b[2] for b in blocks], [b[3] for b in blocks], rates, common_sr,
                                                      n_fft, hop, offsets=offsets, row_strides=[b[4] for b in blocks])
        n_frames, first_frame = plan["n_frames"].copy(), plan["first_frame"].copy()
        total = tot["n_frames"]
        out = self.empty((total, n_mels) if frame_major else (total * n_mels,))
        bad = self.zeros((n,), dtype=torch.int32)
        if n == 0:
            return out, n_frames, first_frame, bad
        table = np.concatenate([plan.view(np.uint8), order.view(np.uint8)])
        table_dev = torch.from_numpy(table).to(self.device)
        self.frontend_bytes += table.nbytes
        plan_ptr, order_ptr = _vp(table_dev.data_ptr()), _vp(table_dev.data_ptr() + plan.nbytes)
        mono = self.empty((max(tot["mono_floats"], 4),))
        if pad_value is not None:
            mono.fill_(pad_value)
        totals = np.zeros(1, np.dtype(_lib.FRONTEND_TOTALS_FIELDS))
        for name, v in tot.items():
            totals[0][name] = v
        with torch.cuda.device(self.device):
            for g in range(len(groups)):
                _lib.check(self.lib.at_mix_resample_ragged_f32(
                    self.ctx.handle, _vp(base), plan_ptr, order_ptr, _vp(groups.ctypes.data + g * groups.itemsize),
                    _ptr(mono), self._stream()))
                self.frontend_calls += 1
            logmel_ragged = self.lib.at_logmel_ragged_minmax_f32 if minmax else self.lib.at_logmel_ragged_f32
            _lib.check(logmel_ragged(
                self.ctx.handle, _ptr(mono), plan_ptr, n, _np_ptr(totals), common_sr, n_fft, hop, n_mels, _ptr(fbt),
                _ptr(out), _lib.AT_LAYOUT_FRAME_MAJOR if frame_major else _lib.AT_LAYOUT_MEL_MAJOR, 1 if l2norm else 0,
                _ptr(bad), self._stream()))
            self.frontend_calls += 1
        self.frontend_last = {"mono": mono, "plan": plan, "order": order, "groups": groups, "totals": tot}
        return out, n_frames, first_frame, bad

    def flac_decode(self, blobs):
        """FLAC files (bytes each) -> per blob, in order, (float32 [C, L] device tensor, sample_rate), the values
        torchaudio.load returns, or None for a blob that did not index or decode.  One index pass on the host, ONE upload
        (the files back to back and the frame table behind them) and three stream operations whatever the number of clips.
        self.flac_status then holds, per blob, 0, the negative AT_E_FLAC_* code of the indexer or the positive AT_FLAC_*
        kind of the clip's first failing frame."""
        self.flac_status = status = [0] * len(blobs)
        if not blobs:
            return []
        host, plan = self._flac_pack(blobs, status)
        dev = host.to(self.device, non_blocking=True)
        out, clip_status = self._flac_launch(dev, plan)
        decoded = clip_status.cpu().tolist()                 # (waits for the decode, and so for the upload)
        # the flat buffer and the table of the clips that decoded, in order: what frontend_ragged accepts as `clips`
        self.flac_flat = (out, [(f[2], f[0]["channels"], f[0]["total_samples"])
                                for c, f in enumerate(plan["facts"]) if f is not None and decoded[c] == 0])
        res = []
        for c, f in enumerate(plan["facts"]):
            if f is None:
                res.append(None)
                continue
            status[c] = decoded[c]
            C, L = f[0]["channels"], f[0]["total_samples"]
            res.append((out[f[2]:f[2] + C * L].view(C, L), f[0]["sample_rate"]) if decoded[c] == 0 else None)
        return res

    def _flac_pack(self, blobs, status):
        """Host half of flac_decode: index every blob, then one pinned buffer = the indexed files back to back, 8 zero
        bytes, and (64-byte aligned) the concatenated frame table.  -> (buffer, plan)."""
        facts, tables, pos, base = [], [], 0, 0
        for c, blob in enumerate(blobs):
            try:
                f, fr = self.flac_index(blob)
            except _lib.NativeError as e:
                if e.code not in (_lib.AT_E_FLAC_NOT_FLAC, _lib.AT_E_FLAC_UNSUPPORTED, _lib.AT_E_FLAC_CORRUPT):
                    raise
                status[c] = e.code
                facts.append(None)
                continue
            fr["offset"] += pos
            fr["clip"], fr["out_base"] = c, base
            facts.append((f, pos, base))
            tables.append(fr)
            pos += len(blob)
            base += f["channels"] * f["total_samples"]
        table = np.concatenate(tables) if tables else np.zeros(0, np.dtype(_lib.FLAC_FRAME_FIELDS))
        table_at = (pos + 8 + 63) // 64 * 64
        host = torch.zeros(table_at + table.nbytes, dtype=torch.uint8).pin_memory()
        hv = host.numpy()
        for blob, f in zip(blobs, facts):
            if f is not None:
                hv[f[1]:f[1] + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        hv[table_at:] = table.view(np.uint8)
        return host, {"facts": facts, "data_bytes": pos, "table_at": table_at, "n_frames": len(table),
                      "n_clips": len(blobs), "out_floats": base}

    def _flac_launch(self, dev, plan, out=None):
        """Device half: at_flac_decode_f32 on the uploaded buffer -> (out float32 [out_floats], clip_status int32)."""
        if out is None:
            out = self.empty(max(plan["out_floats"], 1))
        frame_status = self.empty(max(plan["n_frames"], 1), dtype=torch.int32)
        clip_status = self.empty(plan["n_clips"], dtype=torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_flac_decode_f32(_ptr(dev), plan["data_bytes"], _vp(dev.data_ptr() + plan["table_at"]),
                                                   plan["n_frames"], plan["n_clips"], _ptr(out), plan["out_floats"],
                                                   _ptr(frame_status), _ptr(clip_status), self._stream()))
        return out, clip_status

    def token_histogram(self, ids, k: int) -> torch.Tensor:
        """int64 [k] counts of the token ids (device tensor in, device tensor out)."""
        if isinstance(ids, np.ndarray):
            ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64))
        ids = ids.to(self.device, dtype=torch.int64).contiguous().reshape(-1)
        counts = self.empty((k,), torch.int64)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_token_histogram_i64(self.ctx.handle, _ptr(ids), ids.numel(), k, _ptr(counts), self._stream()))
        return counts

    def token_stats(self, counts):
        """counts: int64 [k] device histogram -> (sorted_counts int64 [k] descending, sorted_tokens int32 [k],
        stats float64 [8]: total, unique, ranks below 80 % cumulative share, slope, intercept, r, points fitted), all on
        the device (at_token_stats_f64)."""
        assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.device == self.device
        k = counts.numel()
        sc, stok = self.empty((k,), torch.int64), self.empty((k,), torch.int32)
        stats = self.empty((8,), torch.float64)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_token_stats_f64(self.ctx.handle, _ptr(counts), k, _ptr(sc), _ptr(stok), _ptr(stats), self._stream()))
        return sc, stok, stats

    def minmax_scale_clips(self, specs) -> torch.Tensor:
        """specs [n_clips, ...] float32 on the device: every clip becomes (x - min) / (max - min), in place."""
        assert specs.dtype == torch.float32 and specs.is_contiguous() and specs.device == self.device
        if specs.shape[0]:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.at_minmax_scale_clips_f32(self.ctx.handle, _ptr(specs), specs.shape[0],
                                                              specs[0].numel(), self._stream()))
        return specs

    def conv1d_mel(self, frames, weight, bias=None, padding=1) -> torch.Tensor:
        """frames [n, n_mels] -> [n, n_mels * num_kernels]: nn.Conv1d(1, num_kernels, kernel_size, padding) along the mel
        axis, feature = mel * num_kernels + kernel (at_conv1d_mel_f32).  weight: the module's [num_kernels, 1, kernel_size]."""
        frames = self._f32(frames)
        n, n_mels = frames.shape
        w = self._f32(weight).reshape(weight.shape[0], -1).contiguous()
        b = self._f32(bias).contiguous() if bias is not None else None
        nk, ks = w.shape
        out = self.empty((n, n_mels * nk))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_conv1d_mel_f32(self.ctx.handle, _ptr(frames), n, n_mels, _ptr(w), _ptr(b), nk, ks, int(padding),
                                                  _ptr(out), self._stream()))
        return out

    def l2norm_rows(self, x, out=None) -> torch.Tensor:
        x = self._f32(x)
        assert x.dim() == 2
        n, d = x.shape
        if out is None:
            out = torch.empty_like(x)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_l2norm_rows_f32(self.ctx.handle, _ptr(x), n, d, _ptr(out), self._stream()))
        return out

    def assign(self, x, c, want_dist=True):
        """Nearest centroid under squared L2 (at_assign_f32): x [n, d], c [k, d] -> (ids [n] int64, dist [n] float32 or
        None), the oracle's bits; the lowest index on equal distances.  A centroid is a candidate only at a distance
        below +inf: a row none of whose distances is finite (|x|^2 overflows from finite elements) is (-1, +inf), and a
        centroid whose own norm overflows is never named.  assign_hinted, assign_pruned, assign_c2f and assign_unguided
        return the same for any input, whatever they are hinted."""
        x, c = self._f32(x), self._f32(c)
        assert x.dim() == 2 and c.dim() == 2 and x.shape[1] == c.shape[1]
        n, d = x.shape
        k = c.shape[0]
        ids = self.empty((n,), torch.int64)
        dist = self.empty((n,), torch.float32) if want_dist else None
        rec = self._trace_list("plain")
        if rec is not None:  # bench.py: HIP events on the launch stream around every assign launch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(self.device))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_assign_f32(self.ctx.handle, _ptr(x), n, d, _ptr(c), k, _ptr(ids),
                                              _ptr(dist), self._stream()))
        if rec is not None:
            e1.record(torch.cuda.current_stream(self.device))
            rec.append(("plain", n, d, k, e0, e1))
        return ids, dist

    def knn(self, x, c, k, want_dist=True):
        """The k nearest centroids of every row (at_knn_f32): x [n, d], c [k_c, d] (made float32, contiguous, on the
        device) -> (ids [n, k] int64, dist [n, k] float32 or None), ascending (dis, id); slots with nothing to list are
        (-1, +inf).  Column 0 is assign()'s answer on finite rows.  k < 1 raises RuntimeError."""
        k = int(k)
        if k < 1:
            raise RuntimeError(f"knn: k must be at least 1, got {k}")
        x, c = self._f32(x), self._f32(c)
        assert x.dim() == 2 and c.dim() == 2 and x.shape[1] == c.shape[1]
        n, d = x.shape
        kc = c.shape[0]
        ids = self.empty((n, k), torch.int64)
        dist = self.empty((n, k), torch.float32) if want_dist else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_knn_f32(self.ctx.handle, _ptr(x), n, d, _ptr(c), kc, k, _ptr(ids), _ptr(dist),
                                           self._stream()))
        return ids, dist

    def assign_ip(self, x, c, want_dist=True):
        """The centroid with the largest inner product of every row (at_assign_ip_f32): x [n, d], c [k, d] -> (ids [n]
        int64, ip [n] float32 or None); the lowest index on equal products, (-1, -inf) for a row with nothing to list."""
        x, c = self._f32(x), self._f32(c)
        assert x.dim() == 2 and c.dim() == 2 and x.shape[1] == c.shape[1]
        n, d = x.shape
        ids = self.empty((n,), torch.int64)
        ip = self.empty((n,), torch.float32) if want_dist else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_assign_ip_f32(self.ctx.handle, _ptr(x), n, d, _ptr(c), c.shape[0], _ptr(ids), _ptr(ip),
                                                 self._stream()))
        return ids, ip

    def renorm_rows(self, c) -> torch.Tensor:
        """faiss' fvec_renorm_L2 on the rows of the contiguous float32 device tensor c [k, d], in place
        (at_renorm_rows_f32); returns c."""
        assert c.dim() == 2 and c.dtype == torch.float32 and c.is_contiguous() and c.device == self.device
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_renorm_rows_f32(self.ctx.handle, _ptr(c), c.shape[0], c.shape[1], self._stream()))
        return c

    def pq_encode(self, x, codebooks, want_dist=False):
        """Product-quantiser codes (at_pq_encode_f32): x [n, d], codebooks [M, ksub, d / M] (made float32, contiguous,
        on the device; 1 <= ksub <= 256) -> (codes [n, M] uint8, dist [n, M] float32 or None, bad int32 [1]).
        codes[i, m] is assign()'s answer for the contiguous slice m of x against codebooks[m]; a sub-vector with no
        distance below +inf gets code 0, distance +inf, and sets bad[0].  Nothing is read back."""
        x, cb = self._f32(x), self._f32(codebooks)
        assert x.dim() == 2 and cb.dim() == 3, "pq_encode: x must be [n, d] and codebooks [M, ksub, dsub]"
        n, d = x.shape
        M, ksub, dsub = cb.shape
        if M * dsub != d:
            raise ValueError(f"pq_encode: codebooks {tuple(cb.shape)} do not cut rows of {d} features")
        codes = self.empty((n, M), torch.uint8)
        dist = self.empty((n, M), torch.float32) if want_dist else None
        bad = self.zeros((1,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_pq_encode_f32(self.ctx.handle, _ptr(x), n, d, M, ksub, _ptr(cb), _ptr(codes),
                                                 _ptr(dist), _ptr(bad), self._stream()))
        return codes, dist, bad

    def pq_decode(self, codes, codebooks):
        """codes [n, M] uint8, codebooks [M, ksub, dsub] -> float32 [n, M * dsub]: row codes[i, m] of codebook m, copied
        (at_pq_decode_f32)."""
        cb = self._f32(codebooks)
        if isinstance(codes, np.ndarray):
            codes = torch.from_numpy(np.ascontiguousarray(codes))
        assert codes.dtype == torch.uint8 and codes.dim() == 2 and cb.dim() == 3 and codes.shape[1] == cb.shape[0]
        codes = codes.to(self.device).contiguous()
        n, M = codes.shape
        ksub, dsub = cb.shape[1], cb.shape[2]
        out = self.empty((n, M * dsub))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_pq_decode_f32(self.ctx.handle, _ptr(codes), n, M * dsub, M, ksub, _ptr(cb), _ptr(out),
                                                 self._stream()))
        return out

    def pq_search(self, x, codebooks, codes, k, want_dist=True):
        """The k nearest stored codes of every query by asymmetric distance (at_pq_search_f32): x [n, d], codebooks
        [M, ksub, d / M] (made float32, contiguous, on the device; 1 <= M <= 64, 1 <= ksub <= 256), codes [ntotal, M]
        uint8 (host or device), 1 <= k <= 128 -> (ids [n, k] int64, dist [n, k] float32 or None), ascending (dis, id).
        dis is the sum over m, ascending, of the direct-form distance between sub-vector m of the query and word
        codes[r, m] of codebook m; rows with dis < +inf are listed, the slots left over are (-1, +inf); a row with a
        code >= ksub is never listed.  k < 1 raises RuntimeError.  Nothing is read back."""
        k = int(k)
        if k < 1:
            raise RuntimeError(f"pq_search: k must be at least 1, got {k}")
        x, cb = self._f32(x), self._f32(codebooks)
        if isinstance(codes, np.ndarray):
            codes = torch.from_numpy(np.ascontiguousarray(codes))
        assert x.dim() == 2 and cb.dim() == 3, "pq_search: x must be [n, d] and codebooks [M, ksub, dsub]"
        assert codes.dtype == torch.uint8 and codes.dim() == 2 and codes.shape[1] == cb.shape[0], \
            f"pq_search: codes must be uint8 [ntotal, {cb.shape[0]}]"
        codes = codes.to(self.device).contiguous()
        n, d = x.shape
        M, ksub, dsub = cb.shape
        if M * dsub != d:
            raise ValueError(f"pq_search: codebooks {tuple(cb.shape)} do not cut rows of {d} features")
        ids = self.empty((n, k), torch.int64)
        dist = self.empty((n, k), torch.float32) if want_dist else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_pq_search_f32(self.ctx.handle, _ptr(x), n, d, M, ksub, _ptr(cb), _ptr(codes),
                                                 codes.shape[0], k, _ptr(ids), _ptr(dist), self._stream()))
        return ids, dist

    @staticmethod
    def pq_search_limits(M, ntotal, k) -> dict:
        """include/at_debug.h, at_pq_search_limits: queries per workgroup, database rows per slab and queries per chunk
        of a pq_search() call of that shape (for the tests that sit on those seams)."""
        qb, slab, chunk = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
        _lib.check(_lib.load().at_pq_search_limits(ctypes.byref(qb), ctypes.byref(slab), ctypes.byref(chunk), int(M),
                                                   int(ntotal), int(k)))
        return {"queries_per_block": int(qb.value), "slab_rows": int(slab.value), "queries_per_chunk": int(chunk.value)}

    IVF_TILE_ROWS = 128   # stored rows per tile of the image (csrc/ivf.hip: TILE)

    def ivf_build(self, rows, lists, nlist):
        """The searchable image of an inverted file (at_ivf_build_f32): rows [ntotal, d] float32 and their list numbers
        [ntotal] int64 on the device (outside [0, nlist): in no list) -> an opaque record for ivf_search().  The stable
        order of the rows by list is torch's stable sort; the image is allocated from the host-side bound
        ntotal // 128 + nlist on its tiles.  Nothing is read back."""
        rows = self._f32(rows)
        nlist = int(nlist)
        assert rows.dim() == 2 and lists.dtype == torch.int64 and lists.shape == (rows.shape[0],)
        ntotal, d = rows.shape
        lists = lists.to(self.device).contiguous()
        unlisted = (lists < 0) | (lists >= nlist)
        order = torch.sort(torch.where(unlisted, torch.full_like(lists, nlist), lists), stable=True).indices.contiguous()
        ntiles = ntotal // self.IVF_TILE_ROWS + nlist
        tile_floats = self.IVF_TILE_ROWS * 64 * ((d + 63) // 64) + 256
        img = self.empty((ntiles, tile_floats))
        pos2id = self.empty((ntiles * self.IVF_TILE_ROWS,), torch.int32)
        first = self.empty((nlist + 1,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_ivf_build_f32(self.ctx.handle, _ptr(rows), _ptr(lists), _ptr(order), ntotal, d, nlist,
                                                 ntiles, _ptr(img), _ptr(pos2id), _ptr(first), self._stream()))
        return {"img": img, "pos2id": pos2id, "first": first, "ntiles": ntiles, "ntotal": ntotal, "nlist": nlist, "d": d}

    def ivf_search(self, x, probes, image, k, want_dist=True):
        """The k nearest stored rows among the probed lists (at_ivf_search_f32): x [n, d], probes [n, nprobe] int64 (list
        numbers, distinct within a row; -1: no list), image from ivf_build(), 1 <= k <= 32 -> (ids [n, k] int64, dist
        [n, k] float32 or None), ascending (dis, id), (-1, +inf) in the places left over.  dis is always the expansion
        form of assign().  Queries whose d is no multiple of 4 are padded with +0, which changes no bit.  k < 1 raises
        RuntimeError.  Nothing is read back."""
        k = int(k)
        if k < 1:
            raise RuntimeError(f"ivf_search: k must be at least 1, got {k}")
        x = self._f32(x)
        assert x.dim() == 2 and x.shape[1] == image["d"], f"ivf_search: expected [n, {image['d']}]"
        assert probes.dtype == torch.int64 and probes.dim() == 2 and probes.shape[0] == x.shape[0]
        probes = probes.to(self.device).contiguous()
        n, d = x.shape
        if d % 4:
            x = torch.nn.functional.pad(x, (0, 4 - d % 4)).contiguous()
        ids = self.empty((n, k), torch.int64)
        dist = self.empty((n, k), torch.float32) if want_dist else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_ivf_search_f32(self.ctx.handle, _ptr(x), n, x.shape[1], _ptr(probes), probes.shape[1],
                                                  image["nlist"], _ptr(image["img"]), image["ntiles"],
                                                  _ptr(image["pos2id"]), _ptr(image["first"]), image["ntotal"], k,
                                                  _ptr(ids), _ptr(dist), self._stream()))
        return ids, dist

    IVFPQ_GROUP_ROWS = 16   # rows a list of the grouped codes is padded to (csrc/ivfpq.hip: GROUP)

    def ivfpq_build(self, codes, lists, nlist):
        """The searchable image of PQ codes behind inverted lists (at_ivfpq_build): codes [ntotal, M] uint8 and their list
        numbers [ntotal] int64 on the device (outside [0, nlist): in no list) -> an opaque record for ivfpq_search().
        The stable order of the rows by list is torch's stable sort; everything is allocated from the host-side bound
        ntotal // 16 + nlist on the groups of 16 rows.  Nothing is read back."""
        nlist = int(nlist)
        if isinstance(codes, np.ndarray):
            codes = torch.from_numpy(np.ascontiguousarray(codes))
        assert codes.dtype == torch.uint8 and codes.dim() == 2, "ivfpq_build: codes must be uint8 [ntotal, M]"
        assert lists.dtype == torch.int64 and lists.shape == (codes.shape[0],)
        codes = codes.to(self.device).contiguous()
        ntotal, M = codes.shape
        lists = lists.to(self.device).contiguous()
        unlisted = (lists < 0) | (lists >= nlist)
        order = torch.sort(torch.where(unlisted, torch.full_like(lists, nlist), lists), stable=True).indices.contiguous()
        ngroups = ntotal // self.IVFPQ_GROUP_ROWS + nlist
        grouped = self.empty((ngroups * self.IVFPQ_GROUP_ROWS, M), torch.uint8)
        pos2id = self.empty((ngroups * self.IVFPQ_GROUP_ROWS,), torch.int32)
        first = self.empty((nlist + 1,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_ivfpq_build(self.ctx.handle, _ptr(codes), _ptr(lists), _ptr(order), ntotal, M, nlist,
                                               ngroups, _ptr(grouped), _ptr(pos2id), _ptr(first), self._stream()))
        return {"codes": grouped, "pos2id": pos2id, "first": first, "ngroups": ngroups, "ntotal": ntotal, "nlist": nlist,
                "M": M}

    def ivfpq_search(self, x, probes, centroids, codebooks, image, k, want_dist=True):
        """The k nearest stored codes among the probed lists (at_ivfpq_search_f32): x [n, d], probes [n, nprobe] int64
        (list numbers, distinct within a row; -1: no list), centroids [nlist, d] (the query of a (query, list) pair is
        x - centroid, one fp32 subtraction per feature) or None (the query is x itself), codebooks [M, ksub, d / M],
        image from ivfpq_build(), 1 <= k <= 128 -> (ids [n, k] int64, dist [n, k] float32 or None), ascending
        (dis, id), (-1, +inf) in the places left over.  dis is pq_search()'s: direct-form tables, added in ascending m.
        k < 1 raises RuntimeError.  Nothing is read back."""
        k = int(k)
        if k < 1:
            raise RuntimeError(f"ivfpq_search: k must be at least 1, got {k}")
        x, cb = self._f32(x), self._f32(codebooks)
        assert x.dim() == 2 and cb.dim() == 3, "ivfpq_search: x must be [n, d] and codebooks [M, ksub, dsub]"
        assert probes.dtype == torch.int64 and probes.dim() == 2 and probes.shape[0] == x.shape[0]
        probes = probes.to(self.device).contiguous()
        n, d = x.shape
        M, ksub, dsub = cb.shape
        if M * dsub != d or M != image["M"]:
            raise ValueError(f"ivfpq_search: codebooks {tuple(cb.shape)} do not cut rows of {d} features into {image['M']} codes")
        cent = None
        if centroids is not None:
            cent = self._f32(centroids)
            assert cent.shape == (image["nlist"], d), f"ivfpq_search: centroids must be [{image['nlist']}, {d}]"
        ids = self.empty((n, k), torch.int64)
        dist = self.empty((n, k), torch.float32) if want_dist else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_ivfpq_search_f32(self.ctx.handle, _ptr(x), n, d, _ptr(probes), probes.shape[1],
                                                    image["nlist"], _ptr(cent), M, ksub, _ptr(cb), _ptr(image["codes"]),
                                                    image["ngroups"], _ptr(image["pos2id"]), _ptr(image["first"]),
                                                    image["ntotal"], k, _ptr(ids), _ptr(dist), self._stream()))
        return ids, dist

    @staticmethod
    def ivfpq_search_limits(M, nprobe, k) -> dict:
        """include/at_debug.h, at_ivfpq_search_limits: (query, probe) pairs per workgroup, rows per group of the image
        and queries per chunk of an ivfpq_search() call of that shape (for the tests that sit on those seams)."""
        qb, group, chunk = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
        _lib.check(_lib.load().at_ivfpq_search_limits(ctypes.byref(qb), ctypes.byref(group), ctypes.byref(chunk), int(M),
                                                      int(nprobe), int(k)))
        return {"pairs_per_block": int(qb.value), "rows_per_group": int(group.value), "queries_per_chunk": int(chunk.value)}

    def rq_encode(self, x, codebooks, want_dist=False, want_residual=False):
        """Greedy residual-quantiser codes (at_rq_encode_f32): x [n, d], codebooks [M, ksub, d] (made float32,
        contiguous, on the device; 1 <= ksub <= 256) -> (codes [n, M] uint8, dist [n, M] float32 or None, residual
        [n, d] float32 or None, bad int32 [1]).  Stage m is assign()'s answer for the running residual against
        codebooks[m], then residual -= codebooks[m][code]; a row with no distance below +inf at a stage gets code 0,
        distance +inf, and sets bad[0].  Nothing is read back."""
        x, cb = self._f32(x), self._f32(codebooks)
        assert x.dim() == 2 and cb.dim() == 3, "rq_encode: x must be [n, d] and codebooks [M, ksub, d]"
        n, d = x.shape
        M, ksub, dc = cb.shape
        if dc != d:
            raise ValueError(f"rq_encode: codebooks {tuple(cb.shape)} do not hold rows of {d} features")
        codes = self.empty((n, M), torch.uint8)
        dist = self.empty((n, M), torch.float32) if want_dist else None
        residual = self.empty((n, d), torch.float32) if want_residual else None
        bad = self.zeros((1,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_rq_encode_f32(self.ctx.handle, _ptr(x), n, d, M, ksub, _ptr(cb), _ptr(codes),
                                                 _ptr(dist), _ptr(residual), _ptr(bad), self._stream()))
        return codes, dist, residual, bad

    def rq_beam_step(self, r, b_in, codebook, b_out):
        """One stage of the beam-search residual quantiser (at_rq_beam_step_f32): r [n * b_in, d] or [n, b_in, d], the
        residuals of the b_in beams of every row, codebook [ksub, d] -> (r_out [n, b_out, d] float32, parent [n, b_out]
        int32, code [n, b_out] uint8, dist [n, b_out] float32, bad int32 [1]): the b_out smallest of the rows'
        b_in * min(b_out, ksub) nearest-word candidates by (distance, parent slot, word).  Nothing is read back."""
        r, cb = self._f32(r), self._f32(codebook)
        b_in, b_out = int(b_in), int(b_out)
        d = cb.shape[1]
        assert cb.dim() == 2 and r.shape[-1] == d and b_in >= 1 and r.numel() % (b_in * d) == 0, \
            "rq_beam_step: r must hold [n, b_in, d] floats and codebook [ksub, d]"
        n = r.numel() // (b_in * d)
        r_out = self.empty((n, b_out, d), torch.float32)
        parent = self.empty((n, b_out), torch.int32)
        code = self.empty((n, b_out), torch.uint8)
        dist = self.empty((n, b_out), torch.float32)
        bad = self.zeros((1,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_rq_beam_step_f32(self.ctx.handle, _ptr(r), n, b_in, d, _ptr(cb), cb.shape[0], b_out,
                                                    _ptr(r_out), _ptr(parent), _ptr(code), _ptr(dist), _ptr(bad),
                                                    self._stream()))
        return r_out, parent, code, dist, bad

    def rq_beam_encode(self, x, codebooks, beam, want_dist=False, want_residual=False):
        """Beam-search residual-quantiser codes (at_rq_beam_encode_f32): arguments and results as rq_encode, with a
        beam of 1 <= beam <= 32 partial codes kept alive per row through the stages; the outputs are those of the best
        one behind the last stage.  bad[0] is set when a slot of some stage had no candidate left.  Nothing is read back."""
        x, cb = self._f32(x), self._f32(codebooks)
        assert x.dim() == 2 and cb.dim() == 3, "rq_beam_encode: x must be [n, d] and codebooks [M, ksub, d]"
        n, d = x.shape
        M, ksub, dc = cb.shape
        if dc != d:
            raise ValueError(f"rq_beam_encode: codebooks {tuple(cb.shape)} do not hold rows of {d} features")
        codes = self.empty((n, M), torch.uint8)
        dist = self.empty((n, M), torch.float32) if want_dist else None
        residual = self.empty((n, d), torch.float32) if want_residual else None
        bad = self.zeros((1,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_rq_beam_encode_f32(self.ctx.handle, _ptr(x), n, d, M, ksub, _ptr(cb), int(beam),
                                                      _ptr(codes), _ptr(dist), _ptr(residual), _ptr(bad), self._stream()))
        return codes, dist, residual, bad

    def rq_decode(self, codes, codebooks):
        """codes [n, M] uint8, codebooks [M, ksub, d] -> float32 [n, d]: row codes[i, 0] of codebook 0, then the rows
        codes[i, m] of the codebooks m = 1 .. M-1 added in ascending order (at_rq_decode_f32)."""
        cb = self._f32(codebooks)
        if isinstance(codes, np.ndarray):
            codes = torch.from_numpy(np.ascontiguousarray(codes))
        assert codes.dtype == torch.uint8 and codes.dim() == 2 and cb.dim() == 3 and codes.shape[1] == cb.shape[0]
        codes = codes.to(self.device).contiguous()
        n, M = codes.shape
        ksub, d = cb.shape[1], cb.shape[2]
        out = self.empty((n, d))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_rq_decode_f32(self.ctx.handle, _ptr(codes), n, d, M, ksub, _ptr(cb), _ptr(out),
                                                 self._stream()))
        return out

    def _frame_prefix(self, n_frames, total):
        """Per-clip frame counts -> the device prefix [n_clips + 1] (int64) of at_mfcc_f32 / at_deltas_f32: one upload."""
        counts = np.asarray(n_frames, dtype=np.int64).reshape(-1)
        if (counts < 0).any() or int(counts.sum()) != total:
            raise ValueError(f"the clips hold {int(counts.sum())} frames, the rows {total}")
        prefix = np.zeros(counts.size + 1, np.int64)
        np.cumsum(counts, out=prefix[1:])
        return torch.from_numpy(prefix).to(self.device), counts.size

    def mfcc(self, rows, n_frames, n_mfcc=40, dct=None, orders=0, win_length=5, top_db=None, frame_major=True,
             norm="ortho", out=None):
        """MFCC and delta features of log-mel rows (at_mfcc_f32): rows [n, n_mels] frame-major, as logmel(...,
        frame_major=True) and frontend_ragged leave them; n_frames: the frames of every clip, in order (they add up to
        n; zeros allowed) -> [n, D] (frame_major) or flat [n * D] with clip i a [D, T_i] block at D * first_frame[i];
        D = n_mfcc * (1 + orders), feature o * n_mfcc + k.  top_db: None, or the per-clip clamp of amplitude_to_DB;
        dct: the caller's table [n_mels, n_mfcc] (default: dct_matrix(n_mfcc, n_mels, norm), kept on the device).
        The prefix is built on the host from n_frames: one small upload, nothing is read back."""
        rows = self._f32(rows)
        assert rows.dim() == 2, "mfcc: rows must be [n, n_mels]"
        n, n_mels = rows.shape
        prefix, n_clips = self._frame_prefix(n_frames, n)
        if dct is None:
            cache = self.__dict__.setdefault("_dct_tables", {})
            key = (int(n_mfcc), int(n_mels), norm)
            if key not in cache:
                cache[key] = self.from_host(self.dct_matrix(int(n_mfcc), int(n_mels), norm))
            dct = cache[key]
        else:
            dct = self._f32(dct)
            if tuple(dct.shape) != (n_mels, n_mfcc):
                raise ValueError(f"mfcc: dct must be [n_mels, n_mfcc] = [{n_mels}, {n_mfcc}], got {tuple(dct.shape)}")
        D = int(n_mfcc) * (1 + int(orders)) if 0 <= int(orders) <= 2 else int(n_mfcc)
        if out is None:
            out = self.empty((n, D) if frame_major else (n * D,))
        else:
            assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n * D
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_mfcc_f32(
                self.ctx.handle, _ptr(rows), _ptr(prefix), n_clips, n, n_mels, int(n_mfcc), _ptr(dct), int(orders),
                int(win_length), 0 if top_db is None else 1, 0.0 if top_db is None else float(top_db), _ptr(out),
                _lib.AT_LAYOUT_FRAME_MAJOR if frame_major else _lib.AT_LAYOUT_MEL_MAJOR, self._stream()))
        return out

    def deltas(self, rows, n_frames, win_length=5, out=None):
        """The delta operator of mfcc() alone (at_deltas_f32): rows [n, F] frame-major, n_frames as for mfcc -> [n, F]."""
        rows = self._f32(rows)
        assert rows.dim() == 2, "deltas: rows must be [n, F]"
        n, F = rows.shape
        prefix, n_clips = self._frame_prefix(n_frames, n)
        if out is None:
            out = self.empty((n, F))
        else:
            assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n * F
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_deltas_f32(self.ctx.handle, _ptr(rows), _ptr(prefix), n_clips, n, F, int(win_length),
                                              _ptr(out), self._stream()))
        return out

    def assign_hinted(self, x, c, hint_ids, order=None, want_dist=True):
        """Same result as assign(), faster when the hints (the previous assignment) are mostly right.
        hint_ids: int64 [n] per row.  order: what centroid_accum(..., want_order=True) returned for
        those ids -- a pair (rows in member-list order, their ids in that order), both uint32 bit
        patterns in int32 tensors -- or None.  A hint is only a guess: ids outside [0, k) count as none, and a
        hinted centroid at distance +inf is not an answer (a row with no finite distance is (-1, +inf))."""
        x, c = self._f32(x), self._f32(c)
        n, d = x.shape
        k = c.shape[0]
        assert hint_ids.dtype == torch.int64 and hint_ids.is_contiguous() and hint_ids.numel() == n
        hint_sorted = None
        if order is not None:
            order, hint_sorted = order
            for t in (order, hint_sorted):
                assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n
        ids = self.empty((n,), torch.int64)
        dist = self.empty((n,), torch.float32) if want_dist else None
        rec = self._trace_list("hinted")
        if rec is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(self.device))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_assign_hinted_f32(self.ctx.handle, _ptr(x), n, d, _ptr(c), k, _ptr(hint_ids),
                                                     _ptr(order), _ptr(hint_sorted), _ptr(ids), _ptr(dist),
                                                     self._stream()))
        if rec is not None:
            e1.record(torch.cuda.current_stream(self.device))
            rec.append(("hinted", n, d, k, e0, e1))
        return ids, dist

    # -- exact pruning for Lloyd iterations ---------------------------------------------------
    def group_min_dist(self, c, cperm) -> torch.Tensor:
        """cperm: int32 device tensor [ng*32] (-1 padded) -> dmin float32 [k, ng]: a lower bound of the distance (not
        squared) from centroid p to the nearest member of group g; +inf for a group of padding only, 0 wherever no
        bound can be given (a squared distance that overflows fp32, a table outside the fp16 range under the fp16
        bound kernels): such a group is always visited."""
        c = self._f32(c)
        k, d = c.shape
        assert cperm.dtype == torch.int32 and cperm.is_contiguous() and cperm.numel() % 32 == 0
        ng = cperm.numel() // 32
        dmin = self.empty((k, ng))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_group_min_dist_f32(self.ctx.handle, _ptr(c), k, d, _ptr(cperm), ng, _ptr(dmin),
                                                      self._stream()))
        return dmin

    def visit_order(self, ids, dis, k):
        """Rows sorted by (previous id, previous distance) -> (order, ids in that order), int32
        tensors holding uint32 bit patterns."""
        n = ids.numel()
        assert ids.dtype == torch.int64 and ids.is_contiguous()
        order, hs = self.empty((n,), torch.int32), self.empty((n,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_visit_order_f32(self.ctx.handle, _ptr(ids), _ptr(dis), n, k, _ptr(order), _ptr(hs),
                                                   self._stream()))
        return order, hs

    def visit_order_beside(self, ids, dis, k, sum_out=None):
        """visit_order on a stream of its own (it has its own sort buffers): the caller's stream goes on at
        once and must call the returned function before it uses the result.  sum_out (float64 [1] view): the
        objective sum_i dis[i] is queued on that stream too -- nothing on the caller's stream needs it before the join."""
        main = torch.cuda.current_stream(self.device)
        side = getattr(self, "_order_stream", None)
        if side is None:
            side = self._order_stream = torch.cuda.Stream(self.device)
        side.wait_stream(main)                 # ids / dis are complete on the caller's stream
        with torch.cuda.stream(side):
            if sum_out is not None:
                self.sum_f64(dis, out=sum_out)
                sum_out.record_stream(side)
            out = self.visit_order(ids, dis, k)

        def join(out=out, ids=ids, dis=dis):   # (ids / dis are kept alive until the sort has been waited for)
            torch.cuda.current_stream(self.device).wait_stream(side)
            for t in out:
                t.record_stream(torch.cuda.current_stream(self.device))
            return out
        return join

    def sum_beside(self, dis, sum_out):
        """The objective sum_i dis[i] on the side stream of visit_order_beside; the returned function makes the caller's
        stream wait for it (iterations that sort nothing beside -- short shards, the last iteration)."""
        main = torch.cuda.current_stream(self.device)
        side = getattr(self, "_order_stream", None)
        if side is None:
            side = self._order_stream = torch.cuda.Stream(self.device)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            self.sum_f64(dis, out=sum_out)
            sum_out.record_stream(side)

        def join(dis=dis):
            torch.cuda.current_stream(self.device).wait_stream(side)
        return join

    def prune_stats(self, reset=False):
        """(accumulators computed, accumulators of the dense sweep) over this context's exact pruned
        sweeps so far.  Synchronises."""
        a, t = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self.lib.at_prune_stats(self.ctx.handle, ctypes.byref(a), ctypes.byref(t), 1 if reset else 0))
        return int(a.value), int(t.value)

    def group_means(self, c, cperm) -> torch.Tensor:
        c = self._f32(c)
        k, d = c.shape
        ng = cperm.numel() // 32
        means = self.empty((ng, d))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_group_means_f32(self.ctx.handle, _ptr(c), k, d, _ptr(cperm), ng, _ptr(means),
                                                   self._stream()))
        return means

    def group_neighbours(self, means, nnb=4) -> torch.Tensor:
        """[ng, ceil(ng/32)] bit table: for every group the nnb groups with the nearest means
        (itself included).  Heuristic input of the coarse pass."""
        means = self._f32(means)
        ng, d = means.shape
        gnbr = torch.empty((ng, (ng + 31) // 32), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_group_neighbours_f32(self.ctx.handle, _ptr(means), ng, d, int(nnb), _ptr(gnbr),
                                                        self._stream()))
        return gnbr

    def _nearest_mean(self, x, means):
        """Group of the (approximately) nearest group mean -- a guess, so at d = 64 it is taken from the
        fp16 filter sweep over all groups of means instead of the dense fp32 sweep."""
        n, d = x.shape
        ngm = means.shape[0]
        if d not in (64, 128) or n < 20 or not self.switches["filter"]:
            return self.assign(x, means, want_dist=False)[0]
        key = (n, ngm)
        if getattr(self, "_ident", (None,))[0] != key:
            g8 = (ngm + 31) // 32
            perm = torch.full((g8 * 32,), -1, dtype=torch.int32, device=self.device)
            perm[:ngm] = torch.arange(ngm, dtype=torch.int32, device=self.device)
            every = torch.full((g8, (g8 + 31) // 32), -1, dtype=torch.int32, device=self.device)   # all bits set
            self._ident = (key, torch.arange(n, dtype=torch.int32, device=self.device),
                           torch.zeros(n, dtype=torch.int32, device=self.device), perm, every)
        _, order, zeros, perm, every = self._ident
        return self.assign_pruned(x, means, (order, zeros), perm, every, want_dist=False, mode=1, filter=True)[0]

    def assign_unguided(self, x, c, want_dist=True, cperm=None):
        """Exact nearest centroid by the fp16-split filter sweep with no guesses: every row starts without a running
        best, so every group is visited -- no pruning, but three fp16 MFMA products (and the fp32 redo of the rows the
        error bound cannot settle) instead of the fp32 MFMA sweep.  For tables too small to prune (k < 1024): 1.47 against
        2.53 ms per 4.3 M rows at k = 500 (tools/small_k_probe.py).  Same result as assign().  cperm: a spatial grouping
        of the centroids (group_rows_kd); without one they are grouped as they come -- every group is visited either
        way, but alike centroids in a group let the hi*hi screening drop more tiles (1.47 against 1.75 ms)."""
        x, c = self._f32(x), self._f32(c)
        n, k = x.shape[0], c.shape[0]
        cache = getattr(self, "_unguided", None)
        if cache is None or cache[0].numel() < n:
            cache = self._unguided = (torch.arange(n, dtype=torch.int32, device=self.device),
                                      torch.full((n,), -1, dtype=torch.int32, device=self.device), {})
        if cperm is None:
            cperm = cache[2].get(k)
        if cperm is None:
            ng = (k + 31) // 32
            cperm = torch.full((ng * 32,), -1, dtype=torch.int32, device=self.device)
            cperm[:k] = torch.arange(k, dtype=torch.int32, device=self.device)
            cache[2][k] = cperm
        dmin = self.group_min_dist(c, cperm)     # (also leaves the fp16 image of c in the context: image_current)
        return self.assign_pruned(x, c, (cache[0][:n], cache[1][:n]), cperm, dmin, want_dist=want_dist, filter=True,
                                  image_current=True)

    def assign_coarse(self, x, c, cperm, means, gnbr, want_dist=True):
        """Guesses for rows in their own coherent order (frames of clips): nearest group mean -> its
        neighbour groups -> best centroid among them, one launch (at_assign_coarse_f32)."""
        x, c, means = self._f32(x), self._f32(c), self._f32(means)
        n, d = x.shape
        ng = cperm.numel() // 32
        ids = self.empty((n,), torch.int64)
        dist = self.empty((n,), torch.float32) if want_dist else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_assign_coarse_f32(self.ctx.handle, _ptr(x), n, d, _ptr(c), c.shape[0], _ptr(cperm), ng,
                                                     _ptr(means), _ptr(gnbr), _ptr(ids), _ptr(dist), self._stream()))
        return ids, dist

    def assign_c2f(self, x, c, cperm, dmin, gnbr=None, want_dist=True, coherent=False):
        """Exact nearest centroid without guesses: nearest group mean -> best member of that group
        and its neighbour groups (a guess) -> pruned exact sweep.  Same result as assign().
        coherent: the rows are in an order in which neighbours are alike (frames of clips): the guess
        is then made in one launch without sorting the rows by mean first."""
        x, c = self._f32(x), self._f32(c)
        ng = cperm.numel() // 32
        means = self.group_means(c, cperm)
        if gnbr is None:
            gnbr = self.group_neighbours(means)
        if coherent and x.shape[1] in (64, 128) and self.switches["filter"] and self.switches["c2f_fused"]:
            guess, gdis = self.assign_coarse(x, c, cperm, means, gnbr)
            return self.assign_pruned(x, c, self.visit_order(guess, gdis, c.shape[0]), cperm, dmin, want_dist=want_dist)
        gx = self._nearest_mean(x, means)
        guess, gdis = self.assign_pruned(x, c, self.visit_order(gx, None, ng), cperm, gnbr, mode=1)
        return self.assign_pruned(x, c, self.visit_order(guess, gdis, c.shape[0]), cperm, dmin, want_dist=want_dist)

    def assign_pruned(self, x, c, order, cperm, dmin, want_dist=True, mode=0, filter=None, image_current=False):
        """mode 0: same result as assign() for any input, rows without a finite distance included ((-1, +inf)
        whatever they guessed); `order` = visit_order(...) of the guesses.
        mode 1: best centroid among the groups named by each 32-row tile (order = visit_order of
        group ids) -- a guess generator.
        filter (default: on unless AT_FILTER=0): fp16-split first stage, same bits out.
        image_current: `dmin` was computed by group_min_dist(c, cperm) on these very tensors and nothing
        has used the filter since, so the fp16 image of the centroids need not be rebuilt."""
        x, c = self._f32(x), self._f32(c)
        n, d = x.shape
        if filter is None:
            filter = self.switches["filter"]
        use_filter = bool(filter) and d in (64, 128)
        k = c.shape[0]
        order, hint_sorted = order
        ng = cperm.numel() // 32
        ids = self.empty((n,), torch.int64)
        dist = self.empty((n,), torch.float32) if want_dist else None
        rec = self._trace_list("pruned" if mode == 0 else "coarse")
        # exact filtered calls do their pre-pass (guess distances + group masks) inside the sweep kernel
        fused = use_filter and mode == 0 and self.debug_get("filter_fused") != 0
        with torch.cuda.device(self.device):
            if not fused:  # pre-pass first, so that the events below bracket the sweep kernel only
                _lib.check(self.lib.at_prune_mask_f32(self.ctx.handle, _ptr(x), n, d, _ptr(c), k, _ptr(order),
                                                      _ptr(hint_sorted), ng, _ptr(dmin), mode, self._stream()))
            if rec is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(torch.cuda.current_stream(self.device))
            args = _lib.PrunedArgs(x=x.data_ptr(), n=n, d=d, c=c.data_ptr(), k=k, order=order.data_ptr(),
                                   hint_sorted=hint_sorted.data_ptr(), cperm=cperm.data_ptr(), ng=ng,
                                   bounds=dmin.data_ptr() if dmin is not None else None, guess_only=1 if mode else 0,
                                   use_filter=1 if use_filter else 0, prepass_done=0 if fused else 1,
                                   image_current=1 if image_current else 0, ids=ids.data_ptr(),
                                   dist_or_null=dist.data_ptr() if dist is not None else None)
            _lib.check(self.lib.at_assign_pruned_f32(self.ctx.handle, ctypes.byref(args), self._stream()))
        if rec is not None:
            e1.record(torch.cuda.current_stream(self.device))
            rec.append(("pruned" if mode == 0 else "coarse", n, d, k, e0, e1))
        return ids, dist

    def filter_stats(self, reset=True, timing=False):
        """(rows swept by the fp16-split filter, rows it handed to the fp32 sweep) since the last reset;
        with timing also (summed HIP-event ms of the stage-1 kernel, number of exact sweeps timed,
        32x32 tiles multiplied hi*hi, tiles refined with the lo products)."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        ms, cnt = ctypes.c_double(0.0), ctypes.c_int64(0)
        tiles, refined = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self.lib.at_filter_stats(self.ctx.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(ms),
                                            ctypes.byref(cnt), ctypes.byref(tiles), ctypes.byref(refined),
                                            1 if reset else 0))
        return (a.value, b.value, ms.value, cnt.value, tiles.value, refined.value) if timing else (a.value, b.value)

    def filter_probe(self, x, c, order, cperm, dmin):
        """Test hook: stage 1 only -> (winner ids, approx [n, 2] = (P of the winner, gap to runner-up), listed)."""
        x, c = self._f32(x), self._f32(c)
        n, d = x.shape
        k = c.shape[0]
        order, hint_sorted = order
        ng = cperm.numel() // 32
        ids = self.empty((n,), torch.int64)
        approx = self.empty((n, 2), torch.float32)
        listed = ctypes.c_int64(0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_filter_probe_f32(self.ctx.handle, _ptr(x), n, d, _ptr(c), k, _ptr(order),
                                                    _ptr(hint_sorted), _ptr(cperm), ng, _ptr(dmin), _ptr(ids),
                                                    _ptr(approx), ctypes.byref(listed), self._stream()))
        return ids, approx, listed.value

    def prune_peek(self, n, ng):
        """Test hook: (bd float32 [n], mask int32 [ceil(n/32), ceil(ng/32)] holding uint32 bit patterns) as the preceding
        pre-pass over n rows and ng groups (at_prune_mask_f32, same stream) left them in the context's workspace."""
        bd = self.empty((n,), torch.float32)
        mask = self.empty(((n + 31) // 32, (ng + 31) // 32), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_prune_peek(self.ctx.handle, n, ng, _ptr(bd), _ptr(mask), self._stream()))
        return bd, mask

    def block_sched_install(self, sched) -> None:
        """Test hook: the exact filter sweeps of exactly len(sched) row blocks start their blocks in this order (a
        permutation of range(len(sched)), else refused); None removes it."""
        a = np.ascontiguousarray(sched, dtype=np.uint32) if sched is not None else np.zeros(0, np.uint32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_block_sched_install(self.ctx.handle, a.ctypes.data if a.size else None, a.size))

    def block_sched_peek(self, order, tiles):
        """Test hook: (table int32 [blocks], weights uint8 [ceil(n / 32)]) that visit_order made beside `order` (its
        first output) for row blocks of `tiles` tiles, or None when the context holds no table with that tag."""
        n = order.numel()
        nt = (n + 31) // 32
        table, weight = self.empty(((nt + tiles - 1) // tiles,), torch.int32), self.empty((nt,), torch.uint8)
        found = ctypes.c_int(0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_block_sched_peek(self.ctx.handle, _ptr(order), n, tiles, _ptr(table), _ptr(weight),
                                                    ctypes.byref(found), self._stream()))
        return (table, weight) if found.value else None

    def block_sched_last(self):
        """Test hook: (path, tiles per block, blocks) of the last filter sweep; path 0 = visiting order, 1 = a table made
        beside its order, 2 = the installed schedule."""
        p, t, b = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
        _lib.check(self.lib.at_block_sched_last(self.ctx.handle, ctypes.byref(p), ctypes.byref(t), ctypes.byref(b)))
        return int(p.value), int(t.value), int(b.value)

    def block_sched_limits(self):
        """(rows up to which an exact d = 64 sweep runs one tile per wave, ... two tiles per wave)."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self.lib.at_block_sched_limits(ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def rand_perm_prefix_device(self, n: int, seed: int, m: int) -> torch.Tensor:
        """First m entries of faiss' rand_perm(n, seed) as a device int32 tensor, computed on the device
        (no host work, no upload); same bits as HostHelpers.rand_perm_prefix."""
        out = self.empty((m,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_rand_perm_prefix_device(self.ctx.handle, n, seed, m, _ptr(out), self._stream()))
        return out

    def gather_rows(self, x, idx) -> torch.Tensor:
        x = self._f32(x)
        if isinstance(idx, np.ndarray):
            idx = self.from_host(idx.astype(np.int32, copy=False))
        assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.device == self.device
        m, d = idx.numel(), x.shape[1]
        out = self.empty((m, d))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_gather_rows_f32(self.ctx.handle, _ptr(x), d, _ptr(idx), m, _ptr(out),
                                                   self._stream()))
        return out

    def centroid_accum_join(self):
        """Makes the current stream wait for a long-list accumulation left pending by
        centroid_accum(..., defer_join=True).  Must precede any use of the packed partial."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_centroid_accum_join(self.ctx.handle, self._stream()))

    def centroid_accum(self, x, ids, k, out=None, want_order=False, defer_join=False):
        """Packed partial result [k*d + k]: sums [k, d] followed by counts [k].  With want_order also
        (rows sorted by (id, row), their ids in that order) as int32 tensors holding uint32 bit
        patterns -- the `order` argument of assign_hinted."""
        x = self._f32(x)
        n, d = x.shape
        assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == n
        if out is None:
            out = self.empty((k * d + k,))
        order = self.empty((n,), torch.int32) if want_order else None
        sorted_ids = self.empty((n,), torch.int32) if want_order else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_centroid_accum_defer(self.ctx.handle, 1 if defer_join else 0))
            try:
                _lib.check(self.lib.at_centroid_accum_f32(
                    self.ctx.handle, _ptr(x), n, d, _ptr(ids), k, _ptr(out), _vp(out.data_ptr() + 4 * k * d),
                    _ptr(order), _ptr(sorted_ids), self._stream()))
            except Exception:
                # a failed call must not leave a half-deferred join behind: wait for whatever the side stream
                # was given and go back to the joined form
                self.lib.at_centroid_accum_join(self.ctx.handle, self._stream())
                raise
            finally:
                self.lib.at_centroid_accum_defer(self.ctx.handle, 0)
        return (out, (order, sorted_ids)) if want_order else out

    def centroid_accum_weighted(self, x, w, ids, k, out=None, want_order=False):
        """centroid_accum with a weight per row (at_centroid_accum_weighted_f32): the packed partial holds, per cluster
        and in ascending row order, the chains fmaf(x[i], w[i], .) where centroid_accum has the sums and w[i] + . where
        it has the counts.  Everything runs on the current stream: there is nothing to defer or join.  want_order as
        in centroid_accum."""
        x = self._f32(x)
        n, d = x.shape
        w = self._f32(w)
        assert w.dim() == 1 and w.numel() == n, f"weights must be [{n}]"
        assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == n
        if out is None:
            out = self.empty((k * d + k,))
        order = self.empty((n,), torch.int32) if want_order else None
        sorted_ids = self.empty((n,), torch.int32) if want_order else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_centroid_accum_weighted_f32(
                self.ctx.handle, _ptr(x), _ptr(w), n, d, _ptr(ids), k, _ptr(out), _vp(out.data_ptr() + 4 * k * d),
                _ptr(order), _ptr(sorted_ids), self._stream()))
        return (out, (order, sorted_ids)) if want_order else out

    @staticmethod
    def waccum_limits() -> dict:
        """include/at_debug.h, at_waccum_limits: the member-list lengths at which the weighted accumulation changes its
        path (for the tests that pin them)."""
        v = [ctypes.c_int(0) for _ in range(4)]
        _lib.check(_lib.load().at_waccum_limits(*[ctypes.byref(c) for c in v]))
        return dict(zip(("short_batch", "short_batch_wide", "long_list", "ring_chunk"), (int(c.value) for c in v)))

    def centroid_finalize(self, parts, k, d):
        """parts [n_parts, k*d + k] packed partials (rank order) -> (centroids [k, d], hassign [k])."""
        if parts.dim() == 1:
            parts = parts.unsqueeze(0)
        assert parts.is_contiguous() and parts.shape[1] >= k * d + k   # (a packed partial may carry the objective behind)
        n_parts = parts.shape[0]
        cent = self.empty((k, d))
        hassign = self.empty((k,))
        stride = parts.stride(0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_centroid_finalize_f32(
                self.ctx.handle, _ptr(parts), stride, _vp(parts.data_ptr() + 4 * k * d), stride, n_parts,
                k, d, _ptr(cent), _ptr(hassign), self._stream()))
        return cent, hassign

    def split_clusters_device(self, hassign, cent, n: int, nsplit_out) -> None:
        """faiss split_clusters in place on device tensors (hassign [k], cent [k, d]); nsplit_out: int32 [1]."""
        k, d = cent.shape
        assert hassign.dtype == torch.float32 and cent.dtype == torch.float32 and nsplit_out.dtype == torch.int32
        assert hassign.is_contiguous() and cent.is_contiguous() and hassign.numel() == k
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_split_clusters_f32(self.ctx.handle, d, k, n, _ptr(hassign), _ptr(cent), _ptr(nsplit_out),
                                                      self._stream()))

    def _objective_parts(self, parts, k, d, objs):
        if objs is not None:
            assert objs.dtype == torch.float64 and objs.is_contiguous()
            return _ptr(objs), 1, objs.numel()
        if parts.dim() == 1:
            parts = parts.unsqueeze(0)
        off, total = self.part_layout(k, d)
        assert parts.is_contiguous() and parts.shape[1] == total
        return _vp(parts.data_ptr() + 4 * off), total // 2, parts.shape[0]

    def lloyd_stats(self, hassign, parts, k: int, d: int, stats_row, objs=None) -> None:
        """stats_row (float64 [2]) <- (objective summed in rank order, imbalance).  The per-rank objectives are the
        doubles riding at the end of the packed partials, or -- objs given -- a float64 tensor [n_ranks]."""
        assert stats_row.dtype == torch.float64
        ptr, stride, n_parts = self._objective_parts(parts, k, d, objs)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_lloyd_stats_f64(self.ctx.handle, _ptr(hassign), k, ptr, stride, n_parts, _ptr(stats_row),
                                                   self._stream()))

    def lloyd_stats_split(self, hassign, cent, n: int, nsplit_out, parts, stats_row, objs=None) -> None:
        """lloyd_stats followed by split_clusters_device, one launch (at_lloyd_stats_split_f32)."""
        k, d = cent.shape
        assert stats_row.dtype == torch.float64 and nsplit_out.dtype == torch.int32
        assert hassign.dtype == torch.float32 and cent.dtype == torch.float32
        assert hassign.is_contiguous() and cent.is_contiguous() and hassign.numel() == k
        ptr, stride, n_parts = self._objective_parts(parts, k, d, objs)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_lloyd_stats_split_f32(self.ctx.handle, d, k, n, _ptr(hassign), _ptr(cent), _ptr(nsplit_out),
                                                         ptr, stride, n_parts, _ptr(stats_row), self._stream()))

    def sum_parts(self, parts) -> torch.Tensor:
        """parts [n_parts, m] float32 -> [m]: added in ascending part order (at_sum_parts_f32)."""
        assert parts.dim() == 2 and parts.is_contiguous() and parts.dtype == torch.float32
        out = self.empty((parts.shape[1],))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_sum_parts_f32(self.ctx.handle, _ptr(parts), parts.stride(0), parts.shape[0], parts.shape[1],
                                                 _ptr(out), self._stream()))
        return out

    def to_host_async(self, t: torch.Tensor):
        """-> (pinned host tensor, event): the copy is queued on the current stream, the caller's thread goes on;
        whoever needs the values waits for the event."""
        # pinned buffers are kept (allocating one costs milliseconds and synchronises the device): four per
        # (shape, dtype), handed out in turn -- a reader is long done with a buffer four copies later
        key = (tuple(t.shape), t.dtype)
        pool = self.__dict__.setdefault("_pinned_pool", {})
        slot = pool.get(key)
        if slot is None:
            slot = pool[key] = [[torch.empty(t.shape, dtype=t.dtype).pin_memory() for _ in range(4)], 0]
        h = slot[0][slot[1] % 4]
        slot[1] += 1
        h.copy_(t, non_blocking=True)
        return h, self.record_event()

    def sum_f64(self, v, out=None) -> torch.Tensor:
        """Device double scalar (shape [1]); no synchronisation."""
        v = self._f32(v)
        if out is None:
            out = self.empty((1,), torch.float64)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_sum_f32(self.ctx.handle, _ptr(v), v.numel(), _ptr(out), self._stream()))
        return out

    def nonfinite_flag(self, v) -> torch.Tensor:
        """Device int32 [1]: 1 if any value of v is NaN/Inf.  No synchronisation."""
        v = self._f32(v)
        flag = self.empty((1,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_any_nonfinite_f32(self.ctx.handle, _ptr(v), v.numel(), _ptr(flag),
                                                     self._stream()))
        return flag

    def logmel_nonfinite_take(self) -> torch.Tensor:
        """Device int32 [1]: 1 if a unit-row pass of logmel(..., l2norm=True) since the last call met a frame whose
        squared norm is not finite (a NaN / Inf in it, or squares that overflow: confirm with any_nonfinite).  Clears
        the context's flag.  No synchronisation, and no second read of the frames."""
        flag = self.empty((1,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_logmel_nonfinite_take(self.ctx.handle, _ptr(flag), self._stream()))
        return flag

    def any_nonfinite(self, v) -> bool:
        return bool(self.nonfinite_flag(v).item())

    def silhouette_samples(self, x, labels, sum_out=None) -> torch.Tensor:
        """Exact silhouette of every row (at_silhouette_f32: sklearn's float32 recipe in fp64): x [n, d] rows (made
        float32), labels [n] integers of any values -> device float32 [n] in row order.  sum_out (device float64 [1]),
        if given, receives the fp64 sum of the result.  Raises ValueError, in sklearn's words, for non-finite rows and
        for a label count outside 2 .. n - 1."""
        x = self._f32(x)
        if x.dim() != 2:
            raise ValueError(f"Expected 2D array, got {x.dim()}D array instead")
        if isinstance(labels, np.ndarray):
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64))
        labels = labels.to(self.device, dtype=torch.int64).reshape(-1).contiguous()
        n, d = x.shape
        if labels.numel() != n:
            raise ValueError(f"Found input variables with inconsistent numbers of samples: [{n}, {labels.numel()}]")
        if n < 1 or d < 1:
            raise ValueError(f"Found array with {n} sample(s) and {d} feature(s) while a minimum of 1 is required")
        if self.any_nonfinite(x):
            raise ValueError("Input X contains NaN or infinity.")
        s = self.empty((n,))
        total = sum_out if sum_out is not None else self.empty((1,), torch.float64)
        n_labels = self.empty((1,), torch.int64)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_silhouette_f32(self.ctx.handle, _ptr(x), d, _ptr(labels), n, _ptr(s), _ptr(total),
                                                  _ptr(n_labels), self._stream()))
        k = int(n_labels.item())
        if not 2 <= k <= n - 1:
            raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % k)
        return s

    def _f32_rows(self, t) -> torch.Tensor:
        """A 2-D float32 device view whose rows are contiguous (stride(1) == 1, stride(0) >= the width): strided row
        views pass as they are, anything else (other dtypes, bool / integer labels, host arrays) is converted."""
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t))
        if t.dim() != 2:
            raise ValueError(f"Expected 2D array, got {t.dim()}D array instead")
        if t.device != self.device:
            t = t.to(self.device, non_blocking=t.is_pinned() if t.device.type == "cpu" else True)
        if t.dtype != torch.float32:
            t = t.float()
        if t.shape[0] > 0 and t.shape[1] > 0 and not (t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) >= t.shape[1])):
            t = t.contiguous()
        return t

    def average_precision(self, scores, labels):
        """Exact per-class average precision (at_average_precision_f32: sklearn's average_precision_score per column, in
        fp64): scores, labels [n, c] (made float32 on the device; strided row views are passed by their row stride, not
        copied) -> (ap float64 [c], NaN for the classes without positives; n_pos int64 [c]; map_pair float64 [2] = the sum
        of ap over the classes with positives and their number), device tensors, no synchronisation.  self.ap_flags
        (device int32 [1]) holds the call's flag word: bit 0 a non-finite score, bit 1 a label other than 0 / 1."""
        s, y, ld_s, ld_y, n, c = self._score_label_rows(scores, labels)
        ap = self.empty((c,), torch.float64)
        n_pos = self.empty((c,), torch.int64)
        pair = self.empty((2,), torch.float64)
        self.ap_flags = flags = self.empty((1,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_average_precision_f32(self.ctx.handle, _ptr(s), ld_s, _ptr(y), ld_y, n, c, _ptr(ap),
                                                         _ptr(n_pos), _ptr(pair), _ptr(flags), self._stream()))
        return ap, n_pos, pair

    def _score_label_rows(self, scores, labels):
        """(s, y, ld_s, ld_y, n, c) of a scores / labels pair as the metric entries take them (average_precision's rule)."""
        s, y = self._f32_rows(scores), self._f32_rows(labels)
        if s.shape != y.shape:
            raise ValueError(f"Found input variables with inconsistent shapes: {tuple(y.shape)}, {tuple(s.shape)}")
        n, c = s.shape
        return s, y, (s.stride(0) if n > 1 else c), (y.stride(0) if n > 1 else c), n, c

    def ranking_metrics(self, scores, labels, want_ap=True):
        """Exact per-class ROC AUC and, with want_ap, average precision from one sort per class chunk
        (at_ranking_metrics_f32): scores, labels as for average_precision -> dict of device tensors, no synchronisation:
        auc float64 [c] (NaN without a positive or without a negative), two_u int64 [c] (auc = two_u / (2 P N)), n_pos
        int64 [c], mauc float64 [2] (the sum of the defined auc and their number), and ap float64 [c], map float64 [2]
        (average_precision's bits) or None.  self.ap_flags as for average_precision."""
        s, y, ld_s, ld_y, n, c = self._score_label_rows(scores, labels)
        out = {"auc": self.empty((c,), torch.float64), "two_u": self.empty((c,), torch.int64),
               "n_pos": self.empty((c,), torch.int64), "mauc": self.empty((2,), torch.float64),
               "ap": self.empty((c,), torch.float64) if want_ap else None,
               "map": self.empty((2,), torch.float64) if want_ap else None}
        self.ap_flags = flags = self.empty((1,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_ranking_metrics_f32(
                self.ctx.handle, _ptr(s), ld_s, _ptr(y), ld_y, n, c, _ptr(out["ap"]) if want_ap else None,
                _ptr(out["map"]) if want_ap else None, _ptr(out["auc"]), _ptr(out["two_u"]), _ptr(out["n_pos"]),
                _ptr(out["mauc"]), _ptr(flags), self._stream()))
        return out

    def threshold_counts(self, scores, labels, threshold):
        """Per-class counts of predicted = scores > threshold (strict, in float32) against the labels
        (at_threshold_counts_f32): -> device int64 [c, 3] = tp, fp, fn; no synchronisation.  self.tc_flags (device int32
        [1]) holds the call's flag word, bits as for average_precision."""
        s, y, ld_s, ld_y, n, c = self._score_label_rows(scores, labels)
        counts = self.empty((c, 3), torch.int64)
        self.tc_flags = flags = self.empty((1,), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.at_threshold_counts_f32(self.ctx.handle, _ptr(s), ld_s, _ptr(y), ld_y, n, c,
                                                        float(threshold), _ptr(counts), _ptr(flags), self._stream()))
        return counts


_default: dict = {}


def default_backend(device=None) -> HipBackend:
    """Process-wide HipBackend per device (creates the at_ctx on first use)."""
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("audio_tokens_amd: no ROCm device visible and there is no CPU fallback")
        idx = torch.cuda.current_device()
    else:
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
    be = _default.get(idx)
    if be is None:
        be = _default[idx] = HipBackend(torch.device("cuda", idx))
    return be
