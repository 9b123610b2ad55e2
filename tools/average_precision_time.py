"""Times at_average_precision_f32 (HipBackend.average_precision: the whole call, flags and mAP pair included) on
synthetic sigmoid scores with about two positives per row, at the sizes MetricsCalculator meets: [2 216, 543] and
[19 944, 543] (balanced_train: validation and training set) and [200 000, 543]; and, where sklearn imports, the
reference's loop (one sklearn.metrics.average_precision_score per class with a positive) on the host of the same machine.
tools/average_precision_time.py [--max-n N] [--out FILE]: one JSON line per case (and into FILE).

expected_bytes is the traffic the call's design implies per element of a chunk: the pack kernel (8 B read, 8 B written),
the radix sort (one 8 B histogram read, then 8 B read + 8 B written per 8-bit pass over the 32 score bits and the class
bits), and the two tile kernels (8 B read each); effective_gbs = expected_bytes / device_s, to hold against the HBM rate."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from audio_tokens_amd.backend import default_backend

C = 543


def expected_bytes(n, c, ws_mb=1024):
    cc = max(1, min(c, (ws_mb << 20) // (16 * n)))
    total = 0
    for c0 in range(0, c, cc):
        cn = min(cc, c - c0)
        passes = math.ceil((32 + math.ceil(math.log2(cn)) if cn > 1 else 32) / 8)
        total += n * cn * (16 + 8 + 16 * passes + 16)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-n", type=int, default=200000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    be = default_backend()
    lines = []
    for n in (2216, 19944, 200000):
        if n > args.max_n:
            continue
        g = torch.Generator(device="cuda")
        g.manual_seed(n)
        scores = torch.sigmoid(torch.randn((n, C), device="cuda", generator=g) * 2 - 3)
        labels = (torch.rand((n, C), device="cuda", generator=g) < 2.0 / C).float()
        be.average_precision(scores, labels)               # warm-up (workspace)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            _, _, pair = be.average_precision(scores, labels)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        dt = float(np.median(ts))
        pair = pair.cpu().numpy()
        eb = expected_bytes(n, C)
        rec = {"case": f"[{n}, {C}]", "n": n, "c": C, "device_s": dt, "mAP": float(pair[0] / pair[1]),
               "classes_with_positives": int(pair[1]), "input_bytes": 8 * n * C, "expected_bytes": eb,
               "effective_gbs": eb / dt / 1e9}
        try:
            from sklearn.metrics import average_precision_score
            yh, sh = labels.cpu().numpy(), scores.cpu().numpy()
            t0 = time.perf_counter()
            aps = [average_precision_score(yh[:, j], sh[:, j]) for j in range(C) if yh[:, j].sum() > 0]
            rec["sklearn_loop_s"] = time.perf_counter() - t0
            rec["sklearn_threads"] = 1                     # a Python loop of single-threaded numpy sorts
            rec["host_cpus_available"] = len(os.sched_getaffinity(0))
            rec["sklearn_mAP"] = float(np.mean(aps))
            rec["speedup_vs_sklearn_loop"] = rec["sklearn_loop_s"] / dt
        except ImportError:
            pass
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
