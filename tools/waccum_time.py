"""Times the weighted centroid sums at_centroid_accum_weighted_f32 (Kmeans.train(x, weights=w)) against the unweighted
at_centroid_accum_f32 of the same build, in the same process and alternating with it, and one weighted Lloyd iteration
against the unweighted one: the numbers of DESIGN.md section 6l.  Rows are seeded random unit vectors, the ids one
assign against k of the rows, the weights uniform in [0.5, 2); n = 2^21, k = 8192, d = 64 and 128.  Call times are
medians of host-synchronised calls (each ends in a device synchronise), with their minimum and maximum.  A Lloyd
iteration is (train(niter = 6) - train(niter = 2)) / 4, which cancels the set-up of a training.  The longest member
list's chain is timed as a call on that cluster's rows alone (k = 1) less a call on a single row: what is left is the
walk of the list.  "skewed" repeats the call timings with one list of 2^15 + 1 members and eight of 3000 planted in
the same ids (the random ids have no list above a few hundred).  The target of section 6l: the weighted call takes no more than twice the unweighted one.
tools/waccum_time.py [--n N] [--k K] [--reps R] [--dims 64,128] [--out FILE]: one JSON line per width."""
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

    def stats(ts):
        return 1e3 * float(np.median(ts)), [1e3 * min(ts), 1e3 * max(ts)]

    def train_seconds(x, d, niter, w):
        km = Kmeans(d, k, niter=niter, backend=be)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return timed(lambda: km.train(x, weights=w) if w is not None else km.train(x))[0]

    for d in (int(v) for v in args.dims.split(",")):
        gen = torch.Generator(device=be.device).manual_seed(1234 + d)
        x = torch.randn((n, d), generator=gen, device=be.device)
        x = be.l2norm_rows(x)
        c = x[torch.randperm(n, generator=gen, device=be.device)[:k]].contiguous()
        w = (torch.rand((n,), generator=gen, device=be.device) * 1.5 + 0.5).contiguous()
        ids, _ = be.assign(x, c)
        lengths = torch.bincount(ids, minlength=k)
        out_w, out_u = be.empty((k * d + k,)), be.empty((k * d + k,))
        be.centroid_accum_weighted(x, w, ids, k, out=out_w, want_order=True)      # warm-up (workspace)
        be.centroid_accum(x, ids, k, out=out_u, want_order=True)
        t_w, t_u = [], []
        for _ in range(args.reps):                                  # alternating, so drift hits both alike
            t_w.append(timed(lambda: be.centroid_accum_weighted(x, w, ids, k, out=out_w, want_order=True))[0])
            t_u.append(timed(lambda: be.centroid_accum(x, ids, k, out=out_u, want_order=True))[0])
        ms_w, mm_w = stats(t_w)
        ms_u, mm_u = stats(t_u)
        # the longest list alone
        cmax = int(lengths.argmax())
        rows = torch.nonzero(ids == cmax).reshape(-1)
        xl, wl = x[rows].contiguous(), w[rows].contiguous()
        zl = torch.zeros(rows.numel(), dtype=torch.int64, device=be.device)
        be.centroid_accum_weighted(xl, wl, zl, 1)
        t_l, t_1 = [], []
        for _ in range(args.reps):
            t_l.append(timed(lambda: be.centroid_accum_weighted(xl, wl, zl, 1))[0])
            t_1.append(timed(lambda: be.centroid_accum_weighted(xl[:1], wl[:1], zl[:1], 1))[0])
        ms_l, mm_l = stats(t_l)
        ms_1, mm_1 = stats(t_1)
        lim = be.waccum_limits()
        rec = {"n": n, "d": d, "k": k, "reps": args.reps,
               "weighted_ms": ms_w, "weighted_ms_min_max": mm_w, "unweighted_ms": ms_u, "unweighted_ms_min_max": mm_u,
               "weighted_over_unweighted": ms_w / ms_u, "target_ratio": 2.0, "target_met": bool(ms_w <= 2.0 * ms_u),
               "longest_list": int(lengths.max()), "lists_over_long_list": int((lengths > lim["long_list"]).sum()),
               "mean_list": float(n) / k, "longest_list_call_ms": ms_l, "longest_list_call_ms_min_max": mm_l,
               "one_row_call_ms": ms_1, "one_row_call_ms_min_max": mm_1, "longest_list_chain_ms": ms_l - ms_1, **lim}
        # the same rows with a skew the random ids do not have: one list of 2^15 + 1 members (every digital-silence
        # frame of a batch) and eight of 3000, which both builds hand to their feature-sliced kernels
        ids_s = ids.clone()
        pick = torch.randperm(n, generator=gen, device=be.device)[:(1 << 15) + 1 + 8 * 3000]
        ids_s[pick[:(1 << 15) + 1]] = 7
        for j in range(8):
            ids_s[pick[(1 << 15) + 1 + 3000 * j:(1 << 15) + 1 + 3000 * (j + 1)]] = 100 + j
        be.centroid_accum_weighted(x, w, ids_s, k, out=out_w, want_order=True)
        be.centroid_accum(x, ids_s, k, out=out_u, want_order=True)
        be.centroid_accum(x, ids_s, k, out=out_u, want_order=True)     # (its early lists start from the second call on)
        t_w, t_u = [], []
        for _ in range(args.reps):
            t_w.append(timed(lambda: be.centroid_accum_weighted(x, w, ids_s, k, out=out_w, want_order=True))[0])
            t_u.append(timed(lambda: be.centroid_accum(x, ids_s, k, out=out_u, want_order=True))[0])
        rows = torch.nonzero(ids_s == 7).reshape(-1)
        xl, wl = x[rows].contiguous(), w[rows].contiguous()
        zl = torch.zeros(rows.numel(), dtype=torch.int64, device=be.device)
        be.centroid_accum_weighted(xl, wl, zl, 1)
        t_l = [timed(lambda: be.centroid_accum_weighted(xl, wl, zl, 1))[0] for _ in range(args.reps)]
        rec["skewed"] = {"longest_list": int(rows.numel()), "weighted_ms": stats(t_w)[0], "weighted_ms_min_max": stats(t_w)[1],
                         "unweighted_ms": stats(t_u)[0], "unweighted_ms_min_max": stats(t_u)[1],
                         "weighted_over_unweighted": stats(t_w)[0] / stats(t_u)[0],
                         "longest_list_call_ms": stats(t_l)[0], "longest_list_call_ms_min_max": stats(t_l)[1],
                         "longest_list_chain_ms": stats(t_l)[0] - ms_1}
        for name, ww in (("weighted", w), ("unweighted", None)):
            train_seconds(x, d, 2, ww)                              # warm-up of every kernel of a training
            per_iter = []
            for _ in range(3):
                per_iter.append((train_seconds(x, d, 6, ww) - train_seconds(x, d, 2, ww)) / 4)
            rec[f"{name}_lloyd_iteration_ms"] = 1e3 * float(np.median(per_iter))
            rec[f"{name}_lloyd_iteration_ms_min_max"] = [1e3 * min(per_iter), 1e3 * max(per_iter)]
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x, c, w
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
