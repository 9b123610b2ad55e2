"""Times the dense inner-product sweep at_assign_ip_f32 (IndexFlatIP.search(x, 1), the search of spherical k-means)
against the plain dense L2 sweep at_assign_f32 at the same shape, in the same process and alternating with it, and one
spherical Lloyd iteration end to end: the numbers of DESIGN.md section 6h.  Rows are seeded random unit vectors and the
centroids k of them, n = 2^21, k = 8192, d = 64 and 128.  Call times are medians of host-synchronised calls (each ends
in a device synchronise).  A Lloyd iteration is (train(niter = 6) - train(niter = 2)) / 4, which cancels the set-up of a
training (finite scan, initial centroids, read-back); the L2 iteration measured the same way is the pruned and
filtered one the product runs.  The FLOP count is 2 d k per row.
tools/ip_sweep_time.py [--n N] [--k K] [--reps R] [--dims 64,128] [--out FILE]: one JSON line per width."""
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

FP32_MFMA_TF = 157.3   # AMD's FP32 matrix spec figure for the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 21)
    ap.add_argument("--k", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dims", default="64,128")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    be = default_backend()
    n, k = args.n, args.k
    lines = []

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def train_seconds(x, d, niter, spherical):
        km = Kmeans(d, k, niter=niter, spherical=spherical, backend=be)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return timed(lambda: km.train(x))[0]

    for d in (int(v) for v in args.dims.split(",")):
        gen = torch.Generator(device=be.device).manual_seed(1234 + d)
        x = torch.randn((n, d), generator=gen, device=be.device)
        x = be.l2norm_rows(x)
        c = x[torch.randperm(n, generator=gen, device=be.device)[:k]].contiguous()
        flop = 2.0 * d * k * n
        ids_ip, _ = be.assign_ip(x, c)                              # warm-up (workspace, LDS limits)
        ids_l2, _ = be.assign(x, c)
        agree = float((ids_ip == ids_l2).float().mean())            # unit rows: the same centroid up to rounding ties
        t_ip, t_l2 = [], []
        for _ in range(args.reps):                                  # alternating, so drift hits both alike
            t_ip.append(timed(lambda: be.assign_ip(x, c))[0])
            t_l2.append(timed(lambda: be.assign(x, c))[0])
        ms_ip, ms_l2 = 1e3 * float(np.median(t_ip)), 1e3 * float(np.median(t_l2))
        rec = {"n": n, "d": d, "k": k, "reps": args.reps, "assign_ip_ms": ms_ip, "assign_l2_ms": ms_l2,
               "assign_ip_ms_min_max": [1e3 * min(t_ip), 1e3 * max(t_ip)],
               "assign_l2_ms_min_max": [1e3 * min(t_l2), 1e3 * max(t_l2)],
               "assign_ip_tflops": flop / (ms_ip * 1e-3) / 1e12, "assign_l2_tflops": flop / (ms_l2 * 1e-3) / 1e12,
               "ip_rate_over_l2_rate": ms_l2 / ms_ip,
               "assign_ip_share_of_fp32_mfma_peak": flop / (ms_ip * 1e-3) / 1e12 / FP32_MFMA_TF,
               "rows_with_the_l2_answer": agree}
        for name, spherical in (("spherical", True), ("l2", False)):
            train_seconds(x, d, 2, spherical)                       # warm-up of every kernel of a training
            per_iter = []
            for _ in range(3):
                per_iter.append((train_seconds(x, d, 6, spherical) - train_seconds(x, d, 2, spherical)) / 4)
            rec[f"{name}_lloyd_iteration_ms"] = 1e3 * float(np.median(per_iter))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x, c
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
