"""Times the device FLAC decoder (HipBackend.flac_decode: at_flac_index_host + at_flac_decode_f32) on a batch of
synth_clips clips of 10 s quantised to 16 bits -- mono at 22 050 Hz and stereo at 44 100 Hz -- encoded the way
libFLAC's default roughly does: fixed predictor of order 2, 4096-sample blocks, a fitted Rice parameter per partition
(partition order 3), independent channels.  The files are made here by a numpy-vectorised writer (tests/flac_ref.py
is pure Python, far too slow for this); --distinct different clips are encoded and repeated to --clips files.

Reported per workload: host index + pack time, upload time (HIP events), kernel time (median of --reps, HIP events),
compressed bytes/s in, samples/s out, and the output write rate beside the 6.29 TB/s achievable HBM figure.  Yardsticks
measured in the same run: the path a user has today for the same audio as 16-bit .wav (_load_audio + upload, over
--wav-clips files, per clip), the log-mel time of the same clips, and -- only if torchaudio imports -- torchaudio.load
of the same .flac files on 16 threads.  A rocprofv3 --kernel-trace --stats run of this tool (with --profile: one decode,
no yardsticks) gives the kernel summary kept in profiles/flac_kernel_stats.csv.
tools/flac_time.py [--clips N] [--distinct D] [--seconds S] [--reps R] [--out FILE] [--profile]: one JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import wave as wave_mod
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

HBM_ACHIEVABLE_TBS = 6.29


def _bits(value, n):
    return ((int(value) >> np.arange(n - 1, -1, -1)) & 1).astype(np.uint8)


def _crc8(data):
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def _crc16_rows(rows, lens):
    """CRC-16 (0x8005, initial value 0) of many byte strings at once.  Leading zero bytes leave a zero CRC unchanged, so
    the strings are right-aligned in one matrix and processed column by column."""
    table = np.zeros(256, np.uint16)
    for i in range(256):
        c = i << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
        table[i] = c
    width = int(max(lens))
    m = np.zeros((len(rows), width), np.uint8)
    for i, r in enumerate(rows):
        m[i, width - len(r):] = r
    crc = np.zeros(len(rows), np.uint16)
    for col in np.ascontiguousarray(m.T):
        crc = (crc << 8) ^ table[(crc >> 8) ^ col]
    return crc


def _subframe_bits(s, porder=3):
    """Fixed order 2, Rice method 0, a fitted parameter per partition -> uint8 array of bits."""
    n = len(s)
    res = s[2:] - 2 * s[1:-1] + s[:-2]
    u = (res << 1) ^ (res >> 63)
    pieces = [_bits(0b00010100, 8), _bits(int(s[0]) & 0xFFFF, 16), _bits(int(s[1]) & 0xFFFF, 16), _bits(0, 2), _bits(porder, 4)]
    psize, at = n >> porder, 0
    for p in range(1 << porder):
        cnt = psize - (2 if p == 0 else 0)
        up = u[at: at + cnt]
        at += cnt
        k0 = max(int(np.log2(up.mean() + 1)), 0)
        k = min(range(max(k0 - 1, 0), min(k0 + 2, 15)), key=lambda kk: int((up >> kk).sum()) + cnt * (1 + kk))
        ends = np.cumsum((up >> k) + 1 + k)
        arr = np.zeros(int(ends[-1]), np.uint8)
        arr[ends - k - 1] = 1
        for b in range(k):
            arr[ends - k + b] = (up >> (k - 1 - b)) & 1
        pieces += [_bits(k, 4), arr]
    return np.concatenate(pieces)


def encode_files(waves, sr, block=4096):
    """waves: int64 [n, C, L] -> n FLAC files (bytes)."""
    n, C, L = waves.shape
    rate = {22050: 6, 44100: 9}[sr]
    bodies, owner = [], []
    for i in range(n):
        for fi, a in enumerate(range(0, L, block)):
            blk = waves[i, :, a: a + block]
            bs = blk.shape[1]
            assert bs >= 16 and bs % 8 == 0 and fi < 128, "the writer keeps to one-byte frame numbers and 8 partitions"
            head = bytes([0xFF, 0xF8, ((12 if bs == block else 7) << 4) | rate, ((C - 1) << 4) | (4 << 1), fi])
            head += (bs - 1).to_bytes(2, "big") if bs != block else b""
            head += bytes([_crc8(head)])
            bits = np.concatenate([_subframe_bits(blk[c]) for c in range(C)])
            bodies.append(np.concatenate([np.frombuffer(head, np.uint8), np.packbits(bits)]))
            owner.append(i)
    crcs = _crc16_rows(bodies, [len(b) for b in bodies])
    frames = [b.tobytes() + int(c).to_bytes(2, "big") for b, c in zip(bodies, crcs)]
    files = []
    for i in range(n):
        mine = [f for f, o in zip(frames, owner) if o == i]
        w = 0
        for v, nb in ((block, 16), (block, 16), (min(map(len, mine)), 24), (max(map(len, mine)), 24), (sr, 20), (C - 1, 3),
                      (15, 5), (L, 36)):
            w = (w << nb) | v
        files.append(b"fLaC" + bytes([0x80, 0, 0, 34]) + w.to_bytes(18, "big") + bytes(16) + b"".join(mine))   # (MD5 0: not computed)
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=5000)
    ap.add_argument("--distinct", type=int, default=40)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wav-clips", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="one decode per workload and nothing else (for rocprofv3)")
    ap.add_argument("--encode-only", action="store_true", help="make the files and check one against the index (no GPU)")
    args = ap.parse_args()
    from audio_tokens_amd.synth import synth_clips
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    workloads = []
    for name, C, sr in (("mono_22050", 1, 22050), ("stereo_44100", 2, 44100)):
        L = int(sr * args.seconds) // 8 * 8
        t0 = time.perf_counter()
        w = synth_clips(args.distinct * C, L=L, seed=77 + C, device="cpu").numpy()
        q = np.clip(np.round(w * 32767.0), -32768, 32767).astype(np.int64).reshape(args.distinct, C, L)
        files = encode_files(q, sr)
        emit({"case": name, "stage": "encode", "distinct": args.distinct, "seconds": round(time.perf_counter() - t0, 2),
              "bytes_per_clip": int(np.mean([len(f) for f in files])), "ratio": round(sum(map(len, files)) / (q.size * 2), 3)})
        workloads.append((name, C, sr, L, q, files))
    if args.encode_only:
        from audio_tokens_amd.backend import HostHelpers
        for name, C, sr, L, q, files in workloads:
            facts, table = HostHelpers().flac_index(files[0])
            assert facts["total_samples"] == L and facts["channels"] == C and len(table) == -(-L // 4096), facts
        return

    from audio_tokens_amd.backend import default_backend
    from audio_tokens_amd.processors.spectrogram_generator import _load_audio
    be = default_backend()

    def ev():
        return be.record_event_timed()

    for name, C, sr, L, q, files in workloads:
        blobs = [files[i % len(files)] for i in range(args.clips)]
        # correctness first: the distinct files decode to the samples they were made from
        res = be.flac_decode(files)
        for i, r in enumerate(res):
            assert r is not None and r[1] == sr, (name, i, be.flac_status[i])
            assert torch.equal(r[0].cpu(), torch.from_numpy((q[i] / 32768.0).astype(np.float32))), (name, i)
        del res
        status = [0] * len(blobs)
        t0 = time.perf_counter()
        host, plan = be._flac_pack(blobs, status)
        t_pack = time.perf_counter() - t0
        t0 = time.perf_counter()
        for b in blobs:
            be.flac_index(b)
        t_index = time.perf_counter() - t0
        e0 = ev()
        dev = host.to(be.device, non_blocking=True)
        e1 = ev()
        e1.synchronize()
        t_up = e0.elapsed_time(e1) / 1e3
        out = be.empty(plan["out_floats"])
        times = []
        for _ in range(1 if args.profile else args.reps + 1):           # (the first run warms up)
            a = ev()
            _, cs = be._flac_launch(dev, plan, out=out)
            b = ev()
            b.synchronize()
            times.append(a.elapsed_time(b) / 1e3)
            assert int(cs.abs().sum()) == 0
        t_k = statistics.median(times[1:]) if len(times) > 1 else times[0]
        samples = args.clips * C * L
        emit({"case": name, "stage": "decode", "clips": args.clips, "frames": plan["n_frames"],
              "compressed_bytes": plan["data_bytes"], "samples": samples, "host_index_s": round(t_index, 4),
              "host_index_and_pack_s": round(t_pack, 4), "upload_s": round(t_up, 4), "kernel_s": round(t_k, 5),
              "kernel_runs_s": [round(t, 5) for t in times], "compressed_GB_per_s": round(plan["data_bytes"] / t_k / 1e9, 3),
              "samples_G_per_s": round(samples / t_k / 1e9, 3), "output_write_TB_per_s": round(samples * 4 / t_k / 1e12, 4),
              "hbm_achievable_TB_per_s": HBM_ACHIEVABLE_TBS, "profile_run": bool(args.profile)})
        del dev, host, out
        if args.profile:
            continue

        # yardstick: the same audio as 16-bit .wav through today's path, _load_audio + upload (per clip)
        with tempfile.TemporaryDirectory() as tmp:
            paths = []
            for i in range(len(files)):
                p = Path(tmp) / f"c{i}.wav"
                with wave_mod.open(str(p), "wb") as f:
                    f.setnchannels(C), f.setsampwidth(2), f.setframerate(sr)
                    f.writeframes(np.ascontiguousarray(q[i].T).astype("<i2").tobytes())
                paths.append(p)
                (Path(tmp) / f"c{i}.flac").write_bytes(files[i])
            nw = min(args.wav_clips, args.clips)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = [_load_audio(paths[i % len(paths)])[0].to(be.device) for i in range(nw)]
            torch.cuda.synchronize()
            t_wav = time.perf_counter() - t0
            del keep
            emit({"case": name, "stage": "wav_load_audio_plus_upload", "clips_timed": nw, "seconds": round(t_wav, 4),
                  "per_clip_ms": round(t_wav / nw * 1e3, 4), "scaled_to_clips_s": round(t_wav / nw * args.clips, 3)})
            try:
                import torchaudio
                from concurrent.futures import ThreadPoolExecutor
                fl = [str(Path(tmp) / f"c{i % len(files)}.flac") for i in range(nw)]
                t0 = time.perf_counter()
                with ThreadPoolExecutor(16) as ex:
                    list(ex.map(torchaudio.load, fl))
                t_ta = time.perf_counter() - t0
                emit({"case": name, "stage": "torchaudio_load_16_threads", "clips_timed": nw, "seconds": round(t_ta, 4),
                      "scaled_to_clips_s": round(t_ta / nw * args.clips, 3)})
            except Exception as e:      # not installed (never required)
                emit({"case": name, "stage": "torchaudio_load_16_threads", "skipped": type(e).__name__})

    if not args.profile:
        # yardstick: the log-mel of the same number of 10 s clips at 22 050 Hz (what follows the decode in stage 1)
        L = int(22050 * args.seconds)
        wave = synth_clips(min(args.clips, 512), L=L, seed=5, device="cuda")
        wave = wave.repeat((args.clips + wave.shape[0] - 1) // wave.shape[0], 1)[: args.clips].contiguous()
        outb = be.logmel(wave)
        times = []
        for _ in range(args.reps):
            a = ev()
            be.logmel(wave, out=outb)
            b = ev()
            b.synchronize()
            times.append(a.elapsed_time(b) / 1e3)
        emit({"case": "logmel_22050", "stage": "logmel", "clips": args.clips, "kernel_s": round(statistics.median(times), 5)})
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
