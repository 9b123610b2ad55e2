"""Times ops.IndexIVFFlat -- the lazy build of the searchable image and search(x, k) at several nprobe -- against what a
user had for the same question before it: IndexFlatL2.search(x, k) (at_knn_f32) over the same stored rows, in the same
process and alternating with it.  The numbers of DESIGN.md section 6o; the table goes to profiles/ivf_search.txt.

Data: synthetic frames only, seeded -- unit rows scattered round --centres random unit directions (frames of a corpus
cluster; uniformly random rows would make every list equally far from every query and the recall figure meaningless).
The quantiser is trained by IndexIVFFlat.train on the first 256 * nlist stored rows.  Default shape: ntotal = 2 097 152
rows of d = 64, n = 65 536 queries, nlist = 1024, k = 10, nprobe 1, 8, 32, 128.

Times are CALL times on device inputs: the median of --reps host-synchronised calls (each ends in a device synchronise)
after one warm-up call of the same shape; a search call is the probe search (at_knn_f32 over the centroids) plus
at_ivf_search_f32.  The flat search is timed in the same loop, one call after each IVF call, so both see the same clocks
and neighbours.  recall@k is the share of the flat search's ids (the exact answer) that the IVF search lists for the
same query.  `build` is HipBackend.ivf_build alone (the stable sort of the list numbers and at_ivf_build_f32), `add` the
quantizer.assign of all rows plus the append.

--only-ivf NPROBE runs nothing but --reps IVF searches at that nprobe: the form to put under a kernel trace (a run of
its own), which is where a per-kernel split comes from.

tools/ivf_timing.py [--ntotal 2097152] [--d 64] [--n 65536] [--nlist 1024] [--k 10] [--nprobes 1,8,32,128] [--reps 5]
                    [--centres 4096] [--only-ivf NPROBE] [--out profiles/ivf_search.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from audio_tokens_amd.backend import default_backend
from audio_tokens_amd.ops import IndexFlatL2, IndexIVFFlat


def frames(n, centres, noise, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    pick = torch.randint(0, centres.shape[0], (n,), device=device, generator=g)
    x = centres[pick] + noise * torch.randn(n, centres.shape[1], device=device, generator=g)
    return torch.nn.functional.normalize(x, dim=1).contiguous()


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntotal", type=int, default=2097152)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobes", default="1,8,32,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--noise", type=float, default=0.08, help="per-feature spread of a frame round its centre")
    ap.add_argument("--only-ivf", type=int, default=0, help="run only IVF searches at this nprobe (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "ivf_search.txt"))
    args = ap.parse_args()
    be = default_backend()
    dev = be.device
    nprobes = [int(v) for v in args.nprobes.split(",")]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    g = torch.Generator(device=dev).manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn(args.centres, args.d, device=dev, generator=g), dim=1)
    stored = frames(args.ntotal, centres, args.noise, dev, 2)
    x = frames(args.n, centres, args.noise, dev, 3)

    index = IndexIVFFlat(IndexFlatL2(args.d, backend=be), args.d, args.nlist, backend=be)
    train_ms, _ = timed(lambda: index.train(stored[:256 * args.nlist]))
    add_ms, _ = timed(lambda: index.add(stored, check_finite=False))
    sizes = index.list_sizes

    if args.only_ivf:
        index.nprobe = args.only_ivf
        for _ in range(args.reps + 1):
            timed(lambda: index.search(x, args.k))
        print(f"ran {args.reps + 1} IVF searches at nprobe = {args.only_ivf}")
        return

    timed(lambda: be.ivf_build(index._x, index._lists, args.nlist))          # warm-up
    build = [timed(lambda: be.ivf_build(index._x, index._lists, args.nlist))[0] for _ in range(args.reps)]
    flat = IndexFlatL2(args.d, backend=be)
    flat.add(stored)
    _, (_, exact) = timed(lambda: flat.search(x, args.k))                    # warm-up, and the exact answer

    lines = [f"device: {torch.cuda.get_device_name(dev)}",
             f"ntotal = {args.ntotal} x d = {args.d}, n = {args.n} queries, nlist = {args.nlist}, k = {args.k}; "
             f"{args.centres} latent centres, noise {args.noise}; medians of {args.reps} synchronised calls [min .. max], ms",
             f"list sizes: min {int(sizes.min())}, median {int(statistics.median(sizes.tolist()))}, max {int(sizes.max())}",
             f"train (Kmeans niter = 10 on {256 * args.nlist} rows): {train_ms:.1f} ms, once",
             f"add (quantizer.assign + append): {add_ms:.1f} ms, once",
             f"build (stable sort + at_ivf_build_f32): {statistics.median(build):.2f} [{min(build):.2f} .. {max(build):.2f}]",
             "",
             f"{'nprobe':>7} {'ivf search':>28} {'flat search (at_knn_f32)':>30} {'flat / ivf':>11} {'recall@' + str(args.k):>10}"]
    for nprobe in nprobes:
        index.nprobe = nprobe
        _, (_, ids) = timed(lambda: index.search(x, args.k))                 # warm-up of the shape, and the answer
        hit = ((ids.unsqueeze(2) == exact.unsqueeze(1)) & (exact.unsqueeze(1) >= 0)).any(2)
        recall = float(hit.sum().item()) / max(1, int((exact >= 0).sum().item()))
        del hit, ids
        ti, tf = [], []
        for _ in range(args.reps):                                           # alternating
            ti.append(timed(lambda: index.search(x, args.k))[0])
            tf.append(timed(lambda: flat.search(x, args.k))[0])
        mi, mf = statistics.median(ti), statistics.median(tf)
        lines.append(f"{nprobe:>7} {mi:>9.2f} [{min(ti):>7.2f} .. {max(ti):>7.2f}] {mf:>11.2f} [{min(tf):>7.2f} .. {max(tf):>7.2f}]"
                     f" {mf / mi:>11.2f} {recall:>10.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
