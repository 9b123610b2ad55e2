"""Stage-1 kernel time of one Lloyd-shaped exact call (the set-up of tools/walk_ablate.py) under different starting
orders of its row blocks: the visiting order, its reverse, heaviest first by the TRUE need count (groups per tile from
the stand-alone pre-pass, summed over the tiles of a block: the ceiling of any schedule), and the schedules made from
the distance field of the visiting-order keys (the device's 16 classes; all 256 weights).  Orders alternate within a
round; every figure is one sweep timed by the library's own event pair.
    python tools/sweep_block_order.py [out.txt]      (ROUNDS=8 WARM=4 CLIPS=6000 ITERS=6)
Development aid; profiles/sweep_block_order.txt is its output."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from audio_tokens_amd.backend import default_backend
from audio_tokens_amd.synth import synth_clips

be = default_backend()
be.debug_set("filter_timing", 1)
k = 8192
wave = synth_clips(int(os.environ.get("CLIPS", "6000")), L=220500, seed=4242, device=be.device)
fr = be.logmel(wave, 22050, 512, 128, 64, frame_major=True, l2norm=True)
del wave
g = torch.Generator(device="cuda").manual_seed(1)
x = fr[torch.randperm(fr.shape[0], device="cuda", generator=g)[:2097152]].contiguous()
del fr
n, d = x.shape
c = x[torch.randperm(n, device="cuda", generator=g)[:k]].clone()
for it in range(int(os.environ.get("ITERS", "6"))):
    ids, dis = be.assign(x, c)
    part = be.centroid_accum(x, ids, k)
    c2, h = be.centroid_finalize(part, k, d)
    c = torch.where(h[:, None] > 0, c2, c).contiguous()
cperm = be.from_host(be.group_rows_kd(be.to_host(c)))
dmin = be.group_min_dist(c, cperm)
ng = cperm.numel() // 32
be.debug_set("block_sched", 1)
order = be.visit_order(ids, dis, k)

# the true need count per tile, from the masks of the stand-alone pre-pass
be.debug_set("filter_fused", 0)
ref_ids, ref_dis = be.assign_pruned(x, c, order, cperm, dmin, filter=True)
_, mask = be.prune_peek(n, ng)
be.debug_set("filter_fused", 1)
bits = np.unpackbits(mask.cpu().numpy().view(np.uint8), axis=1).sum(1).astype(np.int64)      # [tiles]
be.assign_pruned(x, c, order, cperm, dmin, filter=True)
_, tiles, blocks = be.block_sched_last()
need = np.add.reduceat(bits, np.arange(0, bits.size, tiles))                                # [blocks]
assert need.size == blocks
table, weight = be.block_sched_peek(order[0], tiles)
table = table.cpu().numpy().view(np.uint32)
w = weight.cpu().numpy().astype(np.int64)
wb = np.maximum.reduceat(w, np.arange(0, w.size, tiles))                                    # block weights

ident = np.arange(blocks, dtype=np.uint32)
orders = {
    "shipped (visiting order)": ("off", None),
    "reversed": ("install", ident[::-1]),
    "heaviest first, true need": ("install", np.argsort(-need, kind="stable").astype(np.uint32)),
    "device table, 16 classes": ("on", None),
    "weights, 256 classes": ("install", np.argsort(-wb, kind="stable").astype(np.uint32)),
    "true need in 16 classes": ("install", np.argsort(-(need * 16 // (need.max() + 1)), kind="stable").astype(np.uint32)),
}


def one(kind, sched):
    be.block_sched_install(sched if kind == "install" else None)
    be.debug_set("block_sched", 0 if kind == "off" else 1)
    be.synchronize()
    be.filter_stats(reset=True)
    got = be.assign_pruned(x, c, order, cperm, dmin, filter=True)
    be.synchronize()
    _, _, ms, sweeps, _, _ = be.filter_stats(timing=True)
    assert sweeps == 1
    assert torch.equal(got[0], ref_ids) and torch.equal(got[1].view(torch.int32), ref_dis.view(torch.int32))
    want = {"off": 0, "on": 1, "install": 2}[kind]
    assert be.block_sched_last()[0] == want, (kind, be.block_sched_last())
    return ms * 1e3


for _ in range(int(os.environ.get("WARM", "4"))):      # every form, until the clocks have settled
    for kind, sched in orders.values():
        one(kind, sched)
rounds = int(os.environ.get("ROUNDS", "8"))
series = {name: [] for name in orders}
for _ in range(rounds):
    for name, (kind, sched) in orders.items():
        series[name].append(one(kind, sched))
be.block_sched_install(None)

lines = [f"# tools/sweep_block_order.py: n={n} d={d} k={k} ng={ng}, {tiles} tiles per block, {blocks} blocks",
         f"# need per block (groups, summed over its tiles): mean {need.mean():.1f}  median {np.median(need):.0f}  "
         f"p90 {np.percentile(need, 90):.0f}  p99 {np.percentile(need, 99):.0f}  max {need.max()} of {tiles * ng}",
         f"# block weights: {np.bincount(wb >> 4, minlength=16).tolist()} blocks per class 0..15; "
         f"rank correlation of weight and true need {np.corrcoef(np.argsort(np.argsort(wb)), np.argsort(np.argsort(need)))[0, 1]:.3f}",
         "# stage-1 kernel, us per sweep; one figure per round, the orders alternating within a round"]
base = series["shipped (visiting order)"]
for name, v in series.items():
    lines.append(f"{name:28s} " + " ".join(f"{t:6.0f}" for t in v) + f"   mean {np.mean(v):6.1f}  min {min(v):6.0f}  max {max(v):6.0f}")
ceil_gain = np.mean(base) - np.mean(series["heaviest first, true need"])
got_gain = np.mean(base) - np.mean(series["device table, 16 classes"])
lines.append(f"# spread of the shipped order {max(base) - min(base):.0f} us; ceiling (true need) {ceil_gain:+.1f} us; "
             f"device table {got_gain:+.1f} us = {100 * got_gain / ceil_gain if ceil_gain else 0:.0f} % of the ceiling")
on = series["device table, 16 classes"]
lines.append(f"# every 'on' run faster than every 'off' run: {max(on) < min(base)}")
text = "\n".join(lines)
print(text, flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
