"""Times the fused residual-quantiser encoder at_rq_encode_f32 against the two compositions it replaces, in the same
process and alternating with them: the numbers of DESIGN.md section 6j and the dispatch rule of
ResidualQuantizer.compute_codes.  (a) per stage one dense be.assign (at_assign_f32, k = 256) and a torch
gather-subtract; (b) per stage one IndexFlatL2.assign (at 128 <= k < 1024 and n >= 65536 the fp16-split filter route)
and the same gather-subtract, the indexes built and warmed before the clock starts.  Rows are seeded random unit
vectors, the codebooks a 3-iteration ResidualQuantizer training of the same rows; every route returns the codes only.
Call times are medians of host-synchronised calls (each ends in a device synchronise) with min and max; the routes are
compared bit for bit first.  The streaming floor is x read once, n * d * 4 bytes at 6.29 TB/s; the flop rate counts
2 n d 256 M against the 157.3 TF fp32 matrix peak.  A second line per shape times one small call, n = 17 230 rows (ten
clips), the way AudioTokenizer would issue it.
tools/rq_time.py [--n N] [--small N] [--reps R] [--shapes 64x4,64x8,128x8] [--out profiles/rq_time.jsonl]: JSON lines."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from audio_tokens_amd.backend import default_backend
from audio_tokens_amd.ops import IndexFlatL2, ResidualQuantizer

HBM_TBS = 6.29      # achievable streaming rate of the MI355X
PEAK_TF = 157.3     # fp32 matrix peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 21)
    ap.add_argument("--small", type=int, default=17230)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="64x4,64x8,128x8")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "rq_time.jsonl"))
    args = ap.parse_args()
    be = default_backend()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    lines = []
    for shape in args.shapes.split(","):
        d, M = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=be.device).manual_seed(d * 100 + M)
        xall = torch.nn.functional.normalize(torch.randn(args.n, d, device=be.device, generator=g), dim=1).contiguous()
        rq = ResidualQuantizer(d, M, niter=3, backend=be)
        rq.train(xall)
        cb = rq.centroids_device
        indexes = []
        for m in range(M):
            index = IndexFlatL2(d, backend=be)
            index.add(cb[m])
            indexes.append(index)

        for n in (args.n, args.small):
            x = xall[:n]

            def fused():
                return be.rq_encode(x, cb)[0]

            def composed_assign():
                r, out = x, []
                for m in range(M):
                    ids, _ = be.assign(r, cb[m], want_dist=False)
                    out.append(ids)
                    if m + 1 < M:
                        r = r - cb[m][ids]
                return out

            def composed_index():
                r, out = x, []
                for m in range(M):
                    ids, _ = indexes[m].assign(r, want_dist=False)
                    out.append(ids)
                    if m + 1 < M:
                        r = r - cb[m][ids]
                return out

            codes = fused()
            same = [all(torch.equal(codes[:, m].to(torch.int64), part[m]) for m in range(M))
                    for part in (composed_assign(), composed_index())]
            taken = rq.compute_codes(x, check_finite=False)
            same.append(bool(torch.equal(taken, codes)))
            del codes, taken
            routes = {"fused": fused, "assign_composition": composed_assign, "index_composition": composed_index,
                      "compute_codes": lambda: rq.compute_codes(x, check_finite=False)}
            times = {name: [] for name in routes}
            for _ in range(args.reps):          # alternating: all see the same clocks and the same neighbours
                for name, fn in routes.items():
                    times[name].append(timed(fn))
            med = {name: statistics.median(v) for name, v in times.items()}
            floor_ms = n * d * 4 / (HBM_TBS * 1e12) * 1e3
            tf = 2.0 * n * d * 256 * M / (med["fused"] * 1e-3) / 1e12
            line = {"n": n, "d": d, "M": M, "reps": args.reps, "what": "call times, host-synchronised, ms",
                    "bit_equal_assign_index_compute_codes": same,
                    **{f"{name}_ms": med[name] for name in routes},
                    **{f"{name}_ms_min_max": [min(times[name]), max(times[name])] for name in routes},
                    "fastest": min(("fused", "assign_composition", "index_composition"), key=lambda k: med[k]),
                    "streaming_floor_ms": floor_ms, "fused_tflops": tf, "fused_share_of_fp32_matrix_peak": tf / PEAK_TF,
                    "kernel_trace": False, "device": torch.cuda.get_device_name(be.device)}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del xall, cb, indexes
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
