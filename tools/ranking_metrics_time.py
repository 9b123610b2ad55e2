"""Times the epoch metrics on synthetic sigmoid scores with about two positives per row, at the sizes MetricsCalculator
meets ([2 216, 543], [19 944, 543], [200 000, 543]; tools/average_precision_time.py's shapes):
  (i)   at_average_precision_f32 alone (HipBackend.average_precision),
  (ii)  at_ranking_metrics_f32 with the average precision (HipBackend.ranking_metrics),
  (iii) at_ranking_metrics_f32 without it (want_ap=False),
  (iv)  at_threshold_counts_f32 (HipBackend.threshold_counts),
  (v)   ops.classification_metrics: (ii) + (iv) and the one host read,
each as the median of host-synchronised calls, the five alternating within a round; and, where sklearn imports, the
reference's host loop for the same six numbers.
tools/ranking_metrics_time.py [--max-n N] [--rounds R] [--no-sklearn] [--out FILE]: one JSON line per case (and into FILE).

expected_bytes_* is the traffic the design implies (tools/average_precision_time.py's model: 136 B per element for (i)
at 543 classes in one chunk; the ROC AUC adds one more 8 B read of the sorted keys; without the average precision its
8 B terms pass goes); the threshold counts read 8 B per element, held against the 6.29 TB/s a streaming read achieves."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from audio_tokens_amd import ops
from audio_tokens_amd.backend import default_backend
from tools.average_precision_time import expected_bytes

C = 543
THRESHOLD = 0.2
HBM_STREAM_GBS = 6290.0


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _sklearn_loop(yh, sh):
    from sklearn.metrics import average_precision_score, f1_score, hamming_loss, roc_auc_score
    t0 = time.perf_counter()
    live = [j for j in range(C) if yh[:, j].sum() > 0]
    aps = [average_precision_score(yh[:, j], sh[:, j]) for j in live]
    aucs = [roc_auc_score(yh[:, j], sh[:, j]) for j in live if yh[:, j].sum() < len(yh)]
    pred = sh > THRESHOLD
    out = {"mAP": float(np.mean(aps)), "mAUC": float(np.mean(aucs)), "d_prime": ops.d_prime(float(np.mean(aucs))),
           "f1_score_micro": float(f1_score(yh, pred, average="micro", zero_division=0)),
           "f1_score_macro": float(f1_score(yh, pred, average="macro", zero_division=0)),
           "hamming_loss": float(hamming_loss(yh, pred))}
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-n", type=int, default=200000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-sklearn", action="store_true", help="skip the host loop (profiling runs)")
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
        calls = {"ap_alone_s": lambda: be.average_precision(scores, labels),
                 "combined_s": lambda: be.ranking_metrics(scores, labels),
                 "auc_only_s": lambda: be.ranking_metrics(scores, labels, want_ap=False),
                 "threshold_counts_s": lambda: be.threshold_counts(scores, labels, THRESHOLD),
                 "classification_metrics_s": lambda: ops.classification_metrics(labels, scores, THRESHOLD, backend=be)}
        for fn in calls.values():                              # warm-up (workspace, code objects)
            _timed(fn)
        ts = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                ts[k].append(_timed(fn))
        rec = {"case": f"[{n}, {C}]", "n": n, "c": C, "rounds": args.rounds}
        rec.update({k: float(np.median(v)) for k, v in ts.items()})
        rec.update({k[:-2] + "_min_s": float(np.min(v)) for k, v in ts.items()})
        eb = expected_bytes(n, C)
        rec["combined_over_ap_alone"] = rec["combined_s"] / rec["ap_alone_s"]
        rec["auc_only_over_ap_alone"] = rec["auc_only_s"] / rec["ap_alone_s"]
        rec["expected_bytes_ap_alone"] = eb
        rec["expected_bytes_combined"] = eb + 8 * n * C
        rec["expected_ratio_combined"] = (eb + 8 * n * C) / eb
        rec["threshold_counts_bytes"] = 8 * n * C
        rec["threshold_counts_gbs"] = 8 * n * C / rec["threshold_counts_s"] / 1e9
        rec["threshold_counts_share_of_stream_rate"] = rec["threshold_counts_gbs"] / HBM_STREAM_GBS
        rec["metrics"] = ops.classification_metrics(labels, scores, THRESHOLD, backend=be)
        try:
            if args.no_sklearn:
                raise ImportError
            rec["sklearn_loop_s"], rec["sklearn_metrics"] = _sklearn_loop(labels.cpu().numpy(), scores.cpu().numpy())
            rec["sklearn_threads"] = 1                         # Python loops of single-threaded numpy sorts
            rec["host_cpus_available"] = len(os.sched_getaffinity(0))
            rec["speedup_vs_sklearn_loop"] = rec["sklearn_loop_s"] / rec["classification_metrics_s"]
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
