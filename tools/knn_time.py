"""Times at_knn_f32 (IndexFlatL2.search(x, k)) on synth_clips frames (log-mel, unit rows) against centroids from a
k = 8192 Kmeans of the same frames: n = 2^21, d = 64 and 128, k in 2, 8, 32, 33, 128, 1024.  In the same process and
alternating with it: at_assign_f32 at the same shape (the k = 1 floor) and the torch composition (fp32 x @ c.T and
torch.topk, chunked so the distance block stays at 1 GiB) with the share of rows on which it agrees with the exact
answer.  Times are medians of host-synchronised calls; kernel times come from a separate rocprofv3 --kernel-trace
--stats run of this tool.
tools/knn_time.py [--n N] [--reps R] [--ks 2,8,...] [--dims 64,128] [--out FILE]: one JSON line per case."""
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

FP32_MFMA_TF = 157.3   # AMD's FP32 matrix spec figure for the MI355X


def torch_topk(x, c, k, chunk=32768):
    cn = (c * c).sum(1)
    I = torch.empty((x.shape[0], k), dtype=torch.int64, device=x.device)
    D = torch.empty((x.shape[0], k), dtype=torch.float32, device=x.device)
    for i0 in range(0, x.shape[0], chunk):
        xb = x[i0:i0 + chunk]
        dis = ((xb * xb).sum(1, keepdim=True) + cn[None, :]) - 2.0 * (xb @ c.T)
        D[i0:i0 + chunk], I[i0:i0 + chunk] = torch.topk(dis.clamp_min_(0), k, dim=1, largest=False, sorted=True)
    return D, I


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", default="2,8,32,33,128,1024")
    ap.add_argument("--dims", default="64,128")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    be = default_backend()
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    kc = 8192
    for d in (int(v) for v in args.dims.split(",")):
        wave = synth_clips(1300, device="cuda")
        frames = be.logmel(wave, n_mels=d, frame_major=True, l2norm=True)
        del wave
        x = frames[:args.n].contiguous()
        del frames
        km = Kmeans(d, kc, niter=5, backend=be)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            km.train(x)
        c = km.centroids_device.contiguous()
        n = x.shape[0]
        flop = 2.0 * d * kc * n
        for k in (int(v) for v in args.ks.split(",")):
            be.knn(x, c, k)                                     # warm-up (workspace, LDS limits)
            be.assign(x, c)
            t_knn, t_k1, t_torch = [], [], []
            for _ in range(args.reps):                          # alternating, so drift hits all three alike
                dt, (I, D) = timed(lambda: be.knn(x, c, k))
                t_knn.append(dt)
                t_k1.append(timed(lambda: be.assign(x, c))[0])
                dt, (Dt, It) = timed(lambda: torch_topk(x, c, k))
                t_torch.append(dt)
            ms, ms1, mst = (1e3 * float(np.median(t)) for t in (t_knn, t_k1, t_torch))
            agree = float((It == I).all(1).float().mean())
            emit({"case": f"n={n} d={d} k_c={kc} k={k}", "n": n, "d": d, "k_c": kc, "k": k,
                  "path": "fused" if k <= 32 else "general", "knn_ms": ms, "assign_k1_ms": ms1, "torch_topk_ms": mst,
                  "ratio_to_k1": ms / ms1, "speedup_vs_torch": mst / ms, "knn_tflops": flop / (ms * 1e-3) / 1e12,
                  "share_of_fp32_mfma_peak": flop / (ms * 1e-3) / 1e12 / FP32_MFMA_TF,
                  "torch_rows_agreeing": agree})
            del I, D, Dt, It
        del x, c, km
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
