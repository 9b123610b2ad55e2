"""Times ops.IndexIVFPQ -- the build of the grouped codes and search(x, k) at several nprobe, with and without residuals
-- against the only route over codes the library had before it, IndexPQ.search over the same rows (encoded with the
codebooks of the by_residual=False index), in the same process and alternating with it, and beside IndexIVFFlat.search
at the same nprobe.  The numbers of DESIGN.md section 6p; the table goes to profiles/ivfpq_search.txt.

The workload is that of tools/ivf_timing.py, so the rows of the two tables can be read side by side: frames are unit
vectors scattered round `--centres` latent centres (torch generator, fixed seeds); the coarse quantiser is trained by
IndexIVFFlat.train on the first 256 * nlist stored rows and shared by all three indexes; the product quantisers are
trained on the same rows (their residuals, or the rows themselves).  Default shape: ntotal = 2 097 152 x d = 64,
n = 65 536 queries, nlist = 1024, k = 10, M in {8, 16}, nprobe in {1, 8, 32, 128}.

Every figure is the median of --reps host-synchronised calls [min .. max] after a warm-up call of the same shape: the
search times include the probe search (backend.knn over the centroids), which is also timed alone.  recall@k is the
share of IndexFlatL2.search's ids on the raw rows (the exact answer) that a search lists for the same query.  The three
memory figures are the bytes of the raw fp32 rows, of what IndexIVFFlat keeps (rows, list numbers, image, tables) and of
what IndexIVFPQ keeps (codes in id order, list numbers, grouped codes, tables, codebooks).

--only-ivfpq NPROBE runs nothing but --reps searches of the by_residual index at that nprobe and the first M: the form
to put under a kernel trace (a run of its own), which gives the split into inversion, scan and merge.

tools/ivfpq_timing.py [--ntotal 2097152] [--d 64] [--n 65536] [--nlist 1024] [--k 10] [--Ms 8,16] [--nprobes 1,8,32,128]
                      [--reps 5] [--centres 4096] [--only-ivfpq NPROBE] [--out profiles/ivfpq_search.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from audio_tokens_amd.backend import default_backend
from audio_tokens_amd.ops import IndexFlatL2, IndexIVFFlat, IndexIVFPQ, IndexPQ


def frames(n, centres, noise, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    pick = torch.randint(0, centres.shape[0], (n,), device=device, generator=g)
    x = centres[pick] + noise * torch.randn(n, centres.shape[1], device=device, generator=g)
    return torch.nn.functional.normalize(x, dim=1).contiguous()


def nbytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors if t is not None)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntotal", type=int, default=2097152)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--Ms", default="8,16")
    ap.add_argument("--nprobes", default="1,8,32,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--noise", type=float, default=0.08, help="per-feature spread of a frame round its centre")
    ap.add_argument("--only-ivfpq", type=int, default=0, help="run only IVFPQ searches at this nprobe (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "ivfpq_search.txt"))
    args = ap.parse_args()
    be = default_backend()
    dev = be.device
    nprobes = [int(v) for v in args.nprobes.split(",")]
    Ms = [int(v) for v in args.Ms.split(",")]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def stat(t):
        return f"{statistics.median(t):>8.2f} [{min(t):>7.2f} .. {max(t):>7.2f}]"

    g = torch.Generator(device=dev).manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn(args.centres, args.d, device=dev, generator=g), dim=1)
    stored = frames(args.ntotal, centres, args.noise, dev, 2)
    x = frames(args.n, centres, args.noise, dev, 3)
    train_rows = stored[:256 * args.nlist]

    quantizer = IndexFlatL2(args.d, backend=be)
    ivf = IndexIVFFlat(quantizer, args.d, args.nlist, backend=be)
    ivf.train(train_rows)

    def make(M, by_residual):
        index = IndexIVFPQ(quantizer, args.d, args.nlist, M, by_residual=by_residual, backend=be)
        train_ms, _ = timed(lambda: index.train(train_rows))
        add_ms, _ = timed(lambda: index.add(stored, check_finite=False))
        return index, train_ms, add_ms

    if args.only_ivfpq:
        index, _, _ = make(Ms[0], True)
        index.nprobe = args.only_ivfpq
        for _ in range(args.reps + 1):
            timed(lambda: index.search(x, args.k))
        print(f"ran {args.reps + 1} IVFPQ searches at M = {Ms[0]}, nprobe = {args.only_ivfpq}")
        return

    ivf.add(stored, check_finite=False)
    flat = IndexFlatL2(args.d, backend=be)
    flat.add(stored)
    _, (_, exact) = timed(lambda: flat.search(x, args.k))                    # the exact answer
    del flat
    listed = max(1, int((exact >= 0).sum().item()))

    def recall(ids):
        hit = ((ids.unsqueeze(2) == exact.unsqueeze(1)) & (exact.unsqueeze(1) >= 0)).any(2)
        return float(hit.sum().item()) / listed

    ivf.nprobe = 1
    timed(lambda: ivf.search(x, args.k))                                     # builds the image
    im = ivf._image
    sizes = ivf.list_sizes
    lines = [f"device: {torch.cuda.get_device_name(dev)}",
             f"ntotal = {args.ntotal} x d = {args.d}, n = {args.n} queries, nlist = {args.nlist}, k = {args.k}; "
             f"{args.centres} latent centres, noise {args.noise}; medians of {args.reps} synchronised calls [min .. max], ms",
             f"list sizes: min {int(sizes.min())}, median {int(statistics.median(sizes.tolist()))}, max {int(sizes.max())}",
             f"memory, MiB: raw fp32 rows {nbytes(stored) / 2**20:.1f}; IndexIVFFlat "
             f"{nbytes(ivf._x, ivf._lists, im['img'], im['pos2id'], im['first']) / 2**20:.1f}"]
    probe_ms = {}
    for nprobe in nprobes:
        kp = min(nprobe, args.nlist)
        timed(lambda: be.knn(x, quantizer._c, kp, want_dist=False))
        probe_ms[nprobe] = [timed(lambda: be.knn(x, quantizer._c, kp, want_dist=False))[0] for _ in range(args.reps)]
    lines.append("probes alone (backend.knn over the centroids): " +
                 "; ".join(f"nprobe {p}: {stat(t).strip()}" for p, t in probe_ms.items()))

    for M in Ms:
        res, train_r, add_r = make(M, True)
        raw, train_p, add_p = make(M, False)
        pq = IndexPQ(args.d, M, backend=be)                                  # the yardstick: every code, every query
        pq.pq.set_centroids(raw.pq.centroids_device)
        pq.add_codes(raw.codes)
        timed(lambda: be.ivfpq_build(res._codes, res._lists, args.nlist))    # warm-up
        build = [timed(lambda: be.ivfpq_build(res._codes, res._lists, args.nlist))[0] for _ in range(args.reps)]
        res.nprobe = 1
        timed(lambda: res.search(x[:16], args.k))
        ri = res._image
        mem = nbytes(res._codes, res._lists, ri["codes"], ri["pos2id"], ri["first"], res.pq.centroids_device, quantizer._c)
        _, (_, ids) = timed(lambda: pq.search(x, args.k))                    # warm-up, and the ceiling of the recall
        lines += ["",
                  f"M = {M}: IndexIVFPQ {mem / 2**20:.1f} MiB; train pq {train_r:.1f} ms (residuals) / {train_p:.1f} ms (rows), "
                  f"add {add_r:.1f} / {add_p:.1f} ms, once; build (stable sort + at_ivfpq_build): {stat(build).strip()}; "
                  f"IndexPQ.search recall@{args.k} {recall(ids):.4f}",
                  f"{'nprobe':>7} {'ivfpq, residuals':>29} {'recall':>7} {'ivfpq, rows':>29} {'recall':>7} "
                  f"{'IndexPQ.search':>29} {'pq / ivfpq':>11} {'IndexIVFFlat':>29}"]
        del ids
        for nprobe in nprobes:
            res.nprobe = raw.nprobe = ivf.nprobe = nprobe
            _, (_, ids) = timed(lambda: res.search(x, args.k))               # warm-up of the shape, and the answer
            rec_r = recall(ids)
            _, (_, ids) = timed(lambda: raw.search(x, args.k))
            rec_p = recall(ids)
            del ids
            timed(lambda: ivf.search(x, args.k))
            tr, tp, ty, tf = [], [], [], []
            for _ in range(args.reps):                                       # alternating
                tr.append(timed(lambda: res.search(x, args.k))[0])
                ty.append(timed(lambda: pq.search(x, args.k))[0])
                tp.append(timed(lambda: raw.search(x, args.k))[0])
                tf.append(timed(lambda: ivf.search(x, args.k))[0])
            lines.append(f"{nprobe:>7} {stat(tr):>29} {rec_r:>7.4f} {stat(tp):>29} {rec_p:>7.4f} {stat(ty):>29} "
                         f"{statistics.median(ty) / statistics.median(tr):>11.2f} {stat(tf):>29}")
        del res, raw, pq
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
