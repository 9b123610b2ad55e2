"""Times the fused product-quantiser encoder at_pq_encode_f32 against the composition it replaces -- per sub-space one
contiguous slice copy and one dense at_assign_f32 call (k = 256) -- in the same process and alternating with it: the
numbers of DESIGN.md section 6i.  Rows are seeded random unit vectors, the codebooks 256 random sub-vectors of them per
sub-space, n = 2^21.  Call times are medians of host-synchronised calls (each ends in a device synchronise); the two
routes are compared bit for bit first.  The streaming floor is x read once, n * d * 4 bytes at 6.29 TB/s.
tools/pq_time.py [--n N] [--reps R] [--shapes 64x8,64x4,128x8,128x16] [--out FILE]: one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from audio_tokens_amd.backend import default_backend

HBM_TBS = 6.29   # achievable streaming rate of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="64x8,64x4,128x8,128x16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    be = default_backend()
    n = args.n

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    lines = []
    for shape in args.shapes.split(","):
        d, M = (int(v) for v in shape.split("x"))
        dsub = d // M
        g = torch.Generator(device=be.device).manual_seed(d * 100 + M)
        x = torch.nn.functional.normalize(torch.randn(n, d, device=be.device, generator=g), dim=1).contiguous()
        rows = torch.randint(0, n, (256,), device=be.device, generator=g)
        cb = torch.stack([x[rows, m * dsub:(m + 1) * dsub] for m in range(M)], 0).contiguous()

        def fused():
            return be.pq_encode(x, cb, want_dist=True)

        def composed():
            return [be.assign(x[:, m * dsub:(m + 1) * dsub].contiguous(), cb[m]) for m in range(M)]

        codes, dist, bad = fused()
        parts = composed()
        same = all(torch.equal(codes[:, m].to(torch.int64), parts[m][0])
                   and torch.equal(dist[:, m].contiguous().view(torch.int32), parts[m][1].view(torch.int32)) for m in range(M))
        del codes, dist, parts
        tf, tc = [], []
        for _ in range(args.reps):          # alternating: both see the same clocks and the same neighbours
            tf.append(timed(fused))
            tc.append(timed(composed))
        f_ms, c_ms = statistics.median(tf), statistics.median(tc)
        floor_ms = n * d * 4 / (HBM_TBS * 1e12) * 1e3
        line = {"n": n, "d": d, "M": M, "dsub": dsub, "reps": args.reps, "bit_equal": bool(same), "bad": int(bad.item()),
                "fused_ms": f_ms, "composition_ms": c_ms, "fused_ms_min_max": [min(tf), max(tf)],
                "composition_ms_min_max": [min(tc), max(tc)], "composition_over_fused": c_ms / f_ms,
                "streaming_floor_ms": floor_ms, "floor_share_of_fused": floor_ms / f_ms,
                "fused_tflops": 2.0 * n * d * 256 / (f_ms * 1e-3) / 1e12, "device": torch.cuda.get_device_name(be.device)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del x, cb
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
