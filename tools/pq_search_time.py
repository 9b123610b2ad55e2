"""Times the search over product-quantiser codes, at_pq_search_f32 (be.pq_search), against the only route the library
offered for the same job before it: be.pq_decode(codes) into the [ntotal, d] fp32 matrix followed by be.knn(x, decoded,
k) -- in the same process and alternating with it: the numbers of DESIGN.md section 6n.

Data: seeded random unit rows; the codebooks come from a 3-iteration ProductQuantizer training on 65 536 of them, the
database is ntotal further rows encoded by be.pq_encode, the queries are n more rows.  Times are CALL times: medians of
host-synchronised calls (each ends in a device synchronise), 9 of the new call; the yardstick gets 9 as well unless one
call of it takes more than a second (3) or more than ten seconds (1) -- `yardstick_reps` says which.  For k > 32
at_knn_f32 sorts every key of every row (its general path): measured once, 0.36 s at n * ntotal = 2^26 keys, 96 s at
2^30 and 23 s at 2^32, so a case with k > 32 and more than --yardstick-max-keys (2^28) keys is timed without the
yardstick and its line says so (`yardstick_skipped`); the default grid then finishes in minutes.  The two routes use
different arithmetic (the yardstick measures the decoded row with at_knn_f32's expansion form), so they are compared
for agreement of the id sets per query, never bit for bit: `id_set_agreement` is the mean share of the new call's ids
that the yardstick lists too.  Memory: ntotal * M bytes of codes against ntotal * d * 4 bytes of decoded rows.

The look-up floor beside each line: the scan reads n * ntotal * M table entries of 4 bytes from LDS, with ds_read_b128
for M <= 32 (four queries per read) and ds_read_b64 above (two); both forms move 256 bytes per clock and CU
(MI355X LDS: 64 dwords wide), so floor = n * ntotal * M * 4 / (256 * CUs * clock).  The CUs are read from the device;
the clock is --clock-mhz (2400, the MI355X's engine clock: torch does not report it).  A call with fewer queries than a
read serves still pays for the whole read: `lookup_floor_ms` counts the queries rounded up to the read's width.

--library-only times the new call alone: the form to put under a kernel trace (a run of its own).
tools/pq_search_time.py [--shapes 64x8,128x16] [--ntotals 1048576,16777216] [--ns 1,64,4096] [--ks 1,10,100] [--reps 9]
                        [--clock-mhz 2400] [--yardstick-max-keys 268435456] [--library-only] [--out profiles/pq_search_time.jsonl]: one JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from audio_tokens_amd.backend import default_backend
from audio_tokens_amd.ops import ProductQuantizer

LDS_BYTES_PER_CLK_CU = 256


def unit_rows(n, d, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, device=device, generator=g), dim=1).contiguous()


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x8,128x16")
    ap.add_argument("--ntotals", default="1048576,16777216")
    ap.add_argument("--ns", default="1,64,4096")
    ap.add_argument("--ks", default="1,10,100")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="engine clock the look-up floor is computed for")
    ap.add_argument("--yardstick-max-keys", type=int, default=1 << 28,
                    help="for k > 32 the yardstick is left out of a case with more than this many n * ntotal keys")
    ap.add_argument("--library-only", action="store_true", help="time the new call alone (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "pq_search_time.jsonl"))
    args = ap.parse_args()
    be = default_backend()
    props = torch.cuda.get_device_properties(be.device)
    cus, clock_hz = props.multi_processor_count, args.clock_mhz * 1e6
    ntotals = [int(v) for v in args.ntotals.split(",")]
    ns = [int(v) for v in args.ns.split(",")]
    ks = [int(v) for v in args.ks.split(",")]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for shape in args.shapes.split(","):
            d, M = (int(v) for v in shape.split("x"))
            pq = ProductQuantizer(d, M, niter=3, backend=be)
            pq.train(unit_rows(65536, d, be.device, d * 100 + M))
            cb = pq.centroids_device
            piece = 1 << 20
            codes_all = torch.cat([be.pq_encode(unit_rows(min(piece, max(ntotals) - r0), d, be.device, 7 + r0), cb)[0]
                                   for r0 in range(0, max(ntotals), piece)], 0)
            xall = unit_rows(max(ns), d, be.device, 5)
            for ntotal in ntotals:
                codes = codes_all[:ntotal]
                qb = be.pq_search_limits(M, ntotal, 1)["queries_per_block"]
                for n in ns:
                    x = xall[:n]
                    for k in ks:
                        def new():
                            return be.pq_search(x, cb, codes, k)

                        def yardstick():
                            return be.knn(x, be.pq_decode(codes, cb), k)

                        ids = new()[0]                       # (warm-up of the shape as well)
                        line = {"d": d, "M": M, "ntotal": ntotal, "n": n, "k": k, "reps": args.reps,
                                "codes_bytes": ntotal * M, "decoded_bytes": ntotal * d * 4}
                        ty, reps_y = [], 0
                        # at_knn_f32 sorts every key of a row for k > 32: 96 s for one call at 2^30 keys, hours beyond
                        skip = k > 32 and n * ntotal > args.yardstick_max_keys
                        if skip:
                            line["yardstick_skipped"] = (f"k = {k} > 32 is at_knn_f32's sort of all n * ntotal = {n * ntotal} "
                                                         f"keys, above --yardstick-max-keys {args.yardstick_max_keys}")
                        if not args.library_only and not skip:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            ids_y = yardstick()[0]           # (its first call of the shape: the warm-up, and the answer)
                            torch.cuda.synchronize()
                            warm = (time.perf_counter() - t0) * 1e3
                            hit = (ids.unsqueeze(2) == ids_y.unsqueeze(1)).any(2) & (ids >= 0)
                            line["id_set_agreement"] = float(hit.sum().item()) / max(1, int((ids >= 0).sum().item()))
                            reps_y = args.reps if warm < 1e3 else 3 if warm < 1e4 else 1
                            del ids_y, hit
                        del ids
                        tn = []
                        for r in range(args.reps):           # alternating: both see the same clocks and neighbours
                            tn.append(timed(new))
                            if r < reps_y:
                                ty.append(timed(yardstick))
                        new_ms = statistics.median(tn)
                        served = (n + qb - 1) // qb * qb
                        floor_ms = served * ntotal * M * 4 / (LDS_BYTES_PER_CLK_CU * cus * clock_hz) * 1e3
                        line.update({"pq_search_ms": new_ms, "pq_search_ms_min_max": [min(tn), max(tn)],
                                     "lds_read_bytes": 4 * qb, "lookup_floor_ms": floor_ms,
                                     "floor_share_of_call": floor_ms / new_ms, "cus": cus, "clock_mhz": clock_hz / 1e6,
                                     "device": torch.cuda.get_device_name(be.device)})
                        if ty:
                            y_ms = statistics.median(ty)
                            line.update({"yardstick_ms": y_ms, "yardstick_ms_min_max": [min(ty), max(ty)],
                                         "yardstick_reps": reps_y, "yardstick_over_pq_search": y_ms / new_ms})
                        print(json.dumps(line), flush=True)
                        out.write(json.dumps(line) + "\n")
                        out.flush()
            del codes_all, xall


if __name__ == "__main__":
    main()
