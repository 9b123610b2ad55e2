"""Times the beam-search residual-quantiser encoder at_rq_beam_encode_f32 against the composition it replaces, in the
same process and alternating with it: the numbers of DESIGN.md section 6m and the dispatch rule of
ResidualQuantizer.compute_codes at max_beam_size > 1.  The composition is ResidualQuantizer._encode_by_stages over
_beam_step_composed: per stage one be.knn (at_knn_f32, an entry point this feature does not change), a stable torch
sort on D, a gather and a subtraction, then the walk back through the parents in torch.  The greedy be.rq_encode at the
same shape is the B = 1 baseline.  Rows are seeded random unit vectors, the codebooks a 3-iteration greedy
ResidualQuantizer training of the same rows; every route returns the codes only.  Call times are medians of
host-synchronised calls (each ends in a device synchronise) with min and max; the routes are compared bit for bit first.
The traffic figure of the library route counts, per stage, the residuals read and written (n (B_m + B_{m+1}) d 4 bytes;
the last stage writes none) and the lists written and read (2 n B_m k_m 12 bytes).  A second line per shape and beam
times one small call, n = 17 230 rows (ten clips).  --mse adds the mean squared reconstruction error of a
3-iteration training and encode of the synthetic clips' unit log-mel frames at B = 1, 2, 5, 8 (M = 4).
--library-only times that route alone and --small 0 leaves the small call out: the form to put under a kernel trace
(a run of its own; profiles/rq_beam_kernel_stats.csv).
tools/rq_beam_time.py [--n N] [--small N] [--reps R] [--shapes 64x4,64x8,128x8] [--beams 2,5,8] [--mse]
                      [--library-only] [--out profiles/rq_beam_time.jsonl]: JSON lines."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from audio_tokens_amd.backend import default_backend
from audio_tokens_amd.ops import ResidualQuantizer

HBM_TBS = 6.29      # achievable streaming rate of the MI355X


def stage_bytes(n, d, M, B, ksub=256):
    total, b = 0, 1
    for m in range(M):
        b_out = min(B, b * ksub)
        k = min(b_out, ksub)
        total += n * (b + (b_out if m + 1 < M else 0)) * d * 4 + 2 * n * b * k * 12
        b = b_out
    return total


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 21)
    ap.add_argument("--small", type=int, default=17230)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="64x4,64x8,128x8")
    ap.add_argument("--beams", default="2,5,8")
    ap.add_argument("--mse", action="store_true")
    ap.add_argument("--library-only", action="store_true", help="time the library route alone (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "rq_beam_time.jsonl"))
    args = ap.parse_args()
    be = default_backend()
    beams = [int(v) for v in args.beams.split(",")]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for shape in args.shapes.split(","):
        d, M = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=be.device).manual_seed(d * 100 + M)
        xall = torch.nn.functional.normalize(torch.randn(args.n, d, device=be.device, generator=g), dim=1).contiguous()
        greedy = ResidualQuantizer(d, M, niter=3, backend=be)
        greedy.train(xall)
        cb = greedy.centroids_device
        for B in beams:
            rq = ResidualQuantizer(d, M, max_beam_size=B, backend=be)
            rq.set_centroids(cb)
            for n in (args.n, args.small):
                if n < 1:
                    continue
                x = xall[:n]

                def library():
                    return be.rq_beam_encode(x, cb, B)[0]

                def composed():
                    return rq._encode_by_stages(x, cb, False, False, step=rq._beam_step_composed)[0]

                routes = {"library": library, "knn_composition": composed,
                          "compute_codes": lambda: rq.compute_codes(x, check_finite=False),
                          "greedy_rq_encode": lambda: be.rq_encode(x, cb)[0]}
                if args.library_only:
                    routes = {"library": library}
                codes = library()
                same = None if args.library_only else [bool(torch.equal(codes, composed())),
                                                       bool(torch.equal(codes, routes["compute_codes"]()))]
                del codes
                times = {name: [] for name in routes}
                for _ in range(args.reps):          # alternating: all see the same clocks and the same neighbours
                    for name, fn in routes.items():
                        times[name].append(timed(fn))
                med = {name: statistics.median(v) for name, v in times.items()}
                nbytes = stage_bytes(n, d, M, B)
                emit({"n": n, "d": d, "M": M, "beam": B, "reps": args.reps,
                      "what": "call times, host-synchronised, ms", "bit_equal_composition_compute_codes": same,
                      **{f"{name}_ms": med[name] for name in routes},
                      **{f"{name}_ms_min_max": [min(times[name]), max(times[name])] for name in routes},
                      "fastest": min((k for k in ("library", "knn_composition") if k in med), key=lambda k: med[k]),
                      "library_stage_bytes": nbytes, "library_stage_bytes_floor_ms": nbytes / (HBM_TBS * 1e12) * 1e3,
                      "kernel_trace": False, "device": torch.cuda.get_device_name(be.device)})
        del xall, cb

    if args.mse:
        from audio_tokens_amd.synth import synth_clips
        wave = synth_clips(400, L=22050, seed=4242, device=be.device)
        frames = be.logmel(wave, n_mels=64, frame_major=True, l2norm=True)
        for B in (1, 2, 5, 8):
            rq = ResidualQuantizer(64, 4, niter=3, max_beam_size=B, backend=be)
            rq.train(frames)
            _, dist = rq.compute_codes(frames, return_distances=True)
            emit({"what": "mean squared reconstruction error, unit log-mel frames of the synthetic clips, M = 4, niter = 3",
                  "frames": int(frames.shape[0]), "d": 64, "M": 4, "beam": B,
                  "mse_per_stage": [float(v) for v in dist.double().mean(0).tolist()]})

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
