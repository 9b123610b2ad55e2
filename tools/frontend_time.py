"""Times SpectrogramGenerator.populate_specs on a batch that looks like decoded AudioSet files: --clips synthetic clips
(default 5000), 90 % of them 10 s long and the rest uniform in 1 .. 10 s, rates an even mix of 44.1 kHz and 48 kHz,
half of them stereo.  The clips are made as device tensors and handed to the stage class in place of its file loader,
so no decoder is in the timing: what is timed is the mono mix, the resampler, the log-mel and the copies back.

Reported per setting of SpectrogramGenerator.ragged (where the class has the switch; a checkout from before the ragged
front end has one route, reported as "per_clip"): wall time of populate_specs (first call = warm-up, then the median
and the spread of --reps calls, each bracketed by a device synchronisation), the number of native front-end calls
(resample, logmel, frontend_ragged's launches), and the bytes and number of device->host copies (Tensor.cpu).  With both
routes at hand their spectrograms are compared bit for bit.  The tool runs unchanged on an older checkout: the numbers
for the route before this front end are taken there, the ragged=False setting is only the cross-check.
--normalize times the same call with config.normalize = True (the per-clip min-max scaling): the ragged route on a
checkout that has it there, the per-length route on an older one.
--mode tokens times audio -> token files instead, on the same clips against --vocab random unit centroids:
"tokenize_audio" (SpecTokenizer.tokenize_audio, where the class has it) and "files" (SpectrogramGenerator.run() then
SpecTokenizer.run() through .npy spectrograms, the only route of an older checkout), one timed pass each after a warm-up
pass, with the native front-end calls and the device->host bytes of the pass; the token files of the two are compared
byte for byte.  The spectrogram files of the file route take 441 KB per 10 s clip: choose --clips to fit the disk.
tools/frontend_time.py [--clips N] [--reps R] [--seed S] [--normalize] [--mode specs|tokens] [--vocab K] [--out FILE]:
one JSON line per route."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--normalize", action="store_true")
    ap.add_argument("--mode", choices=("specs", "tokens"), default="specs")
    ap.add_argument("--vocab", type=int, default=1024)
    args = ap.parse_args()
    from audio_tokens_amd.audio_tokens_config import AudioTokensConfig
    from audio_tokens_amd.processors import spectrogram_generator as sg
    from audio_tokens_amd.synth import synth_clips

    rng = np.random.default_rng(args.seed)
    n = args.clips
    seconds = np.where(rng.random(n) < 0.9, 10.0, rng.uniform(1.0, 10.0, n))
    rates = np.where(np.arange(n) % 2 == 0, 44100, 48000)
    chans = np.where(rng.random(n) < 0.5, 2, 1)
    base = synth_clips(64, L=480000, seed=args.seed, device="cuda")          # 10 s at 48 kHz; clips are cut from these rows
    clips = {}
    for i in range(n):
        L = int(seconds[i] * rates[i])
        rows = [(i + c) % 64 for c in range(chans[i])]
        clips[f"clip{i:06d}"] = (base[rows, :L].clone(), int(rates[i]))
    names = sorted(clips)

    tmp = tempfile.mkdtemp()
    Path(tmp, "split.json").write_text(json.dumps({"train": names, "validation": []}))
    cfg = AudioTokensConfig(split_file=str(Path(tmp, "split.json")), audio_source_path=tmp, dest_spec_path=Path(tmp, "spec"),
                            source_spec_path=Path(tmp, "spec"), spectrogram_batch_size=n, normalize=args.normalize,
                            centroids_path=Path(tmp, "centroids.npy"), dest_tokenized_path=str(Path(tmp, "tok")))
    gen = sg.SpectrogramGenerator(cfg)
    gen.find_audio_file = lambda ytid: Path(tmp, ytid + ".dev")
    sg._load_audio = lambda path: clips[Path(path).stem]
    be = gen.spec_transformer.backend

    count = {"native": 0, "d2h_bytes": 0, "d2h_copies": 0}
    for name in ("resample", "logmel", "logmel_minmax"):
        def wrap(f):
            def g(*a, **k):
                count["native"] += 1
                return f(*a, **k)
            return g
        setattr(be, name, wrap(getattr(be, name)))
    real_cpu = torch.Tensor.cpu

    def counting_cpu(t, *a, **k):
        if t.is_cuda:
            count["d2h_bytes"] += t.numel() * t.element_size()
            count["d2h_copies"] += 1
        return real_cpu(t, *a, **k)
    torch.Tensor.cpu = counting_cpu

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    except OSError:
        commit = ""
    if args.mode == "tokens":
        lines = time_tokens(args, cfg, gen, be, count, names, commit, tmp)
        if args.out:
            with open(args.out, "a") as f:
                for rec in lines:
                    f.write(json.dumps(rec) + "\n")
        return
    routes = [("ragged", True), ("ragged_off", False)] if hasattr(sg.SpectrogramGenerator, "ragged") else [("per_clip", None)]
    lines, results = [], {}
    for route, flag in routes:
        if flag is not None:
            gen.ragged = flag
        times = []
        for rep in range(args.reps + 1):
            for k in count:
                count[k] = 0
            calls0 = getattr(be, "frontend_calls", 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            specs = gen.populate_specs(names)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        timed = times[1:]
        rec = {"route": route, "commit": commit, "normalize": args.normalize, "clips": n, "specs": len(specs), "distinct_lengths": len({c[0].shape[1] for c in clips.values()}),
               "warmup_s": round(times[0], 4), "median_s": round(statistics.median(timed), 4), "min_s": round(min(timed), 4),
               "max_s": round(max(timed), 4), "runs_s": [round(t, 4) for t in timed],
               "native_calls": count["native"] + getattr(be, "frontend_calls", 0) - calls0,
               "d2h_copies": count["d2h_copies"], "d2h_bytes": count["d2h_bytes"]}
        results[route] = specs
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if len(results) == 2:
        a, b = results["ragged"], results["ragged_off"]
        same = len(a) == len(b) and all(x["filename"] == y["filename"] and torch.equal(x["spec"], y["spec"]) for x, y in zip(a, b))
        rec = {"route": "cross_check", "commit": commit, "same_bits": bool(same)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        assert same, "the two routes differ"
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def time_tokens(args, cfg, gen, be, count, names, commit, tmp):
    """--mode tokens: audio -> token files, straight and through spectrogram files."""
    from audio_tokens_amd.processors import SpecTokenizer
    c = np.random.default_rng(args.seed).standard_normal((args.vocab, cfg.n_mels)).astype(np.float32)
    np.save(cfg.centroids_path, c / np.linalg.norm(c, axis=1, keepdims=True))
    tok = SpecTokenizer(cfg)
    paths = [gen.find_audio_file(y) for y in names]
    direct = Path(tmp, "direct")

    def files_route():
        gen.run()
        tok.run()

    def direct_route():
        tok.tokenize_audio(paths, direct)
    routes = [("files", files_route)] + ([("tokenize_audio", direct_route)] if hasattr(SpecTokenizer, "tokenize_audio") else [])
    lines = []
    for route, run in routes:
        times = []
        for rep in range(2):       # a warm-up pass, a timed pass
            for k in count:
                count[k] = 0
            calls0 = getattr(be, "frontend_calls", 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        rec = {"route": route, "mode": "tokens", "commit": commit, "normalize": args.normalize, "clips": len(names),
               "vocab": args.vocab, "warmup_s": round(times[0], 4), "timed_s": round(times[1], 4),
               "native_frontend_calls": count["native"] + getattr(be, "frontend_calls", 0) - calls0,
               "d2h_copies": count["d2h_copies"], "d2h_bytes": count["d2h_bytes"]}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if len(routes) == 2:
        a = {p.name: p.read_bytes() for p in Path(cfg.dest_tokenized_path, "train").glob("*.npy")}
        b = {p.name: p.read_bytes() for p in direct.glob("*.npy")}
        rec = {"route": "cross_check", "mode": "tokens", "commit": commit, "same_bytes": a == b, "files": len(a)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        assert a == b, "the two routes wrote different token files"
    return lines


if __name__ == "__main__":
    main()
