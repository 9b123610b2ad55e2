"""Times at_silhouette_f32 (ops.silhouette_score without sampling) on k-means tokens of synth_clips frames:
n = 10 000, 262 144 and 2 097 152 rows at d = 64 (labels from a k = 8192 k-means of the frames), once at d = 640 (the
frames through a 10-kernel Conv1d, as with use_convolution), and sklearn on the CPU at n = 10 000.
tools/silhouette_time.py [--max-n N] [--out FILE]: one JSON line per case (and into FILE)."""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from audio_tokens_amd.backend import default_backend
from audio_tokens_amd.ops import Kmeans
from audio_tokens_amd.synth import synth_clips

FP64_TF = 78.6   # AMD's FP64 matrix spec figure for the MI355X (not measured here)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-n", type=int, default=2097152)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    be = default_backend()
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def device_time(x, lab, reps):
        total = be.empty((1,), torch.float64)
        be.silhouette_samples(x, lab, sum_out=total)           # warm-up (workspace, LDS limit)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            be.silhouette_samples(x, lab, sum_out=total)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), float(total.item()) / x.shape[0]

    n_max = min(args.max_n, 2097152)
    wave = synth_clips(1300, device="cuda")
    frames = be.logmel(wave, frame_major=True, l2norm=True)
    del wave
    x_all = frames[:n_max].contiguous()
    del frames
    km = Kmeans(64, 8192, niter=5, backend=be)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km.train(x_all)
    ids_all, _ = be.assign(x_all, be.l2norm_rows(km.centroids_device))
    torch.cuda.synchronize()

    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    order = torch.randperm(n_max, device="cuda", generator=g)
    for n in (10000, 262144, 2097152):
        if n > n_max:
            continue
        # rows drawn from all the clips (what silhouette_score(..., sample_size=n) hands the kernel)
        x, lab = x_all[order[:n]].contiguous(), ids_all[order[:n]].contiguous()
        reps = 5 if n <= 262144 else 1
        dt, score = device_time(x, lab, reps)
        flop = 128.0 * n * n
        rec = {"case": f"n={n} d=64", "n": n, "d": 64, "labels": int(torch.unique(lab).numel()), "score": score,
               "device_s": dt, "fp64_matrix_bound_s": flop / (FP64_TF * 1e12), "share_of_bound": flop / (FP64_TF * 1e12) / dt}
        if n == 10000:
            try:
                import sklearn.metrics as sk
                xh, lh = x.cpu().numpy(), lab.cpu().numpy()
                t0 = time.perf_counter()
                ref = sk.silhouette_samples(xh, lh)
                rec["sklearn_cpu_s"] = time.perf_counter() - t0
                s = be.to_host(be.silhouette_samples(x, lab))
                rec["bit_identical_share"] = float((s.view(np.uint32) == ref.view(np.uint32)).mean())
                rec["max_abs_diff"] = float(np.abs(s.astype(np.float64) - ref).max())
                rec["rows_scoring_zero"] = float((ref == 0).mean())
            except ImportError:
                rec["sklearn_cpu_s"] = None
        emit(rec)

    n640 = min(262144, n_max)
    w = torch.randn(10, 1, 3, generator=torch.Generator().manual_seed(0))
    x640 = be.conv1d_mel(x_all[order[:n640]], w)
    dt, score = device_time(x640, ids_all[order[:n640]].contiguous(), 1)
    flop = 2.0 * 640 * n640 * n640
    emit({"case": f"n={n640} d=640", "n": n640, "d": 640, "score": score, "device_s": dt,
          "fp64_matrix_bound_s": flop / (FP64_TF * 1e12), "share_of_bound": flop / (FP64_TF * 1e12) / dt})
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
