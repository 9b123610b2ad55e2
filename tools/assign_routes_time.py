"""Times the routes through the fp32 MFMA sweeps of assign.hip, one JSON line per route.

    python tools/assign_routes_time.py --label branch [--out profiles/assign_steps_time.jsonl] [--reps 9]

Each route is called `--warmup` times, then `--reps` times between two device events with the host synchronised before
and after every call; the line holds every call's milliseconds and their median.  To compare two builds, run the tool
once per build in processes of their own (parent, branch, parent) and select the build by the import path: the package
that comes first on PYTHONPATH is the one timed, this checkout's only if there is none.

Routes: be.assign at 2 097 152 x 64 x 8192, 2 097 152 x 128 x 8192 and 1 048 576 x 640 x 8192; be.assign_hinted as
tools/hinted_only.py sets it up (the previous assignment against slightly moved centroids, member-list order) at
d = 64 and 128; be.assign_pruned(filter=False) with 80 % right guesses (the recipe of
test_ab_switches_leave_the_bits_alone) at d = 64 and 128, and at d = 64 with prune_kernel = 0.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # behind PYTHONPATH: see above
import torch

import audio_tokens_amd
from audio_tokens_amd.backend import default_backend

K = 8192


def unit(n, d, g):
    return torch.nn.functional.normalize(torch.randn(n, d, device="cuda", generator=g), dim=1)


def time_calls(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def dense(be, n, d):
    g = torch.Generator(device="cuda").manual_seed(d)
    x, c = unit(n, d, g), unit(K, d, g)
    return lambda: be.assign(x, c)


def hinted(be, n, d):
    g = torch.Generator(device="cuda").manual_seed(0)
    x, c = unit(n, d, g), unit(K, d, g)
    ids, _ = be.assign(x, c)
    _, order = be.centroid_accum(x, ids, K, want_order=True)
    c2 = torch.nn.functional.normalize(c + 0.02 * torch.randn(K, d, device="cuda", generator=g), dim=1)
    return lambda: be.assign_hinted(x, c2, ids, order)


def pruned(be, n, d):
    g = torch.Generator(device="cuda").manual_seed(5 + d)
    centers = unit(K, d, g)
    x = torch.nn.functional.normalize(
        centers[torch.randint(0, K, (n,), device="cuda", generator=g)] + 0.05 * torch.randn(n, d, device="cuda", generator=g), dim=1)
    c = torch.nn.functional.normalize(centers + 0.01 * torch.randn(K, d, device="cuda", generator=g), dim=1)
    c[1000:1010] = c[0:10]
    ids, _ = be.assign(x, c)
    right = torch.rand(n, device="cuda", generator=g) < 0.8
    guess = torch.where(right, ids, torch.randint(0, K, (n,), device="cuda", generator=g)).contiguous()
    cperm = be.from_host(be.group_rows_kd(c.cpu().numpy()))
    dmin = be.group_min_dist(c, cperm)
    order = be.visit_order(guess, None, K)
    return lambda: be.assign_pruned(x, c, order, cperm, dmin, filter=False)


ROUTES = [
    ("assign", 2097152, 64, dense, {}),
    ("assign", 2097152, 128, dense, {}),
    ("assign", 1048576, 640, dense, {}),
    ("assign_hinted", 2097152, 64, hinted, {}),
    ("assign_hinted", 2097152, 128, hinted, {}),
    ("assign_pruned filter=False", 2097152, 64, pruned, {}),
    ("assign_pruned filter=False", 2097152, 128, pruned, {}),
    ("assign_pruned filter=False", 2097152, 64, pruned, {"prune_kernel": 0}),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True)
    ap.add_argument("--out", default="profiles/assign_steps_time.jsonl")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    assert args.warmup >= 3 and args.reps >= 9
    be = default_backend()
    with open(args.out, "a") as out:
        for route, n, d, setup, sw in ROUTES:
            for name, value in sw.items():
                be.debug_set(name, value)
            ms = time_calls(setup(be, n, d), args.warmup, args.reps)
            for name in sw:
                be.debug_set(name, 1)           # prune_kernel's default
            line = {"label": args.label, "route": route, "n": n, "d": d, "k": K, "switches": sw, "ms": [round(v, 4) for v in ms],
                    "median_ms": round(statistics.median(ms), 4)}
            out.write(json.dumps(line) + "\n")
            out.flush()
            print(json.dumps(line), "from", os.path.dirname(audio_tokens_amd.__file__), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
