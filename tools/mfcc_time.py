"""Times the fused MFCC / delta kernel (HipBackend.mfcc, at_mfcc_f32) against the composition a user of the library had
before it, on the same device tensor: torch.matmul with the DCT table, two replicate-padded grouped conv1d calls
(torchaudio's compute_deltas), a cat and the transposes back to frame-major rows -- the numbers of DESIGN.md section 6k.
The two are first compared within the bound the tests use (Higham's gamma_m * sum |terms| for each fp32 chain, carried
through the delta stages), computed in float64 on the device.  Then call times: medians of host-synchronised calls
(each ends in a device synchronise) with min and max, the routes alternating so that all see the same clocks and
neighbours.  "fused" is HipBackend.mfcc as a user calls it (it builds and uploads the clip prefix); "native" is the
same at_mfcc_f32 call with the prefix and the output already on the device, which is what the streaming floor is held
against: 4 * (n_mels + D) bytes per frame at 6.29 TB/s.  These are call times: no kernel trace, no counters.
tools/mfcc_time.py [--reps R] [--out profiles/mfcc_time.jsonl]: JSON lines, one per (frames, shape)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from audio_tokens_amd import _lib
from audio_tokens_amd.backend import default_backend

HBM_TBS = 6.29      # achievable streaming rate of the MI355X (DESIGN.md section 6j uses the same figure)
U = 2.0 ** -24


def gamma(m):
    return m * U / (1 - m * U)


def deltas_torch(c3, N):
    """compute_deltas(mode="replicate") on [B, F, T]."""
    denom = N * (N + 1) * (2 * N + 1) / 3
    Fq = c3.shape[1]
    kernel = torch.arange(-N, N + 1, dtype=c3.dtype, device=c3.device).repeat(Fq, 1, 1)
    return F.conv1d(F.pad(c3, (N, N), mode="replicate"), kernel, groups=Fq) / denom


def composition(x, dct, n_clips, orders, N):
    """[n, n_mels] -> [n, D]: what a user composes in torch on the log-mel rows."""
    c = torch.matmul(x, dct)
    if orders == 0:
        return c
    T = x.shape[0] // n_clips
    parts = [c.view(n_clips, T, -1).transpose(1, 2)]
    for _ in range(orders):
        parts.append(deltas_torch(parts[-1], N))
    return torch.cat(parts, dim=1).transpose(1, 2).reshape(x.shape[0], -1)


def delta_bound(v, b, N, steps):
    """v, b [B, F, T] float64 (exact values, bound of the computed ones) -> (exact deltas, bound of a computed delta whose
    terms pass through at most `steps` fp32 roundings)."""
    denom = N * (N + 1) * (2 * N + 1) / 3
    w = torch.arange(-N, N + 1, dtype=v.dtype, device=v.device)
    vp, mp, bp = (F.pad(t, (N, N), mode="replicate").unfold(2, 2 * N + 1, 1) for t in (v, v.abs() + b, b))
    return (vp * w).sum(-1) / denom, ((bp * w.abs()).sum(-1) + gamma(steps) * (mp * w.abs()).sum(-1)) / denom


def within_bound(x, dct, n_clips, orders, N, fused, composed):
    x64, t64 = x.double(), dct.double()
    T = x.shape[0] // n_clips
    v = (x64 @ t64).view(n_clips, T, -1).transpose(1, 2)
    b = (gamma(x.shape[1]) * (x64.abs() @ t64.abs())).view(n_clips, T, -1).transpose(1, 2)
    exact, ours, theirs = [v], [b], [b]
    for _ in range(orders):
        nv, nb_ours = delta_bound(exact[-1], ours[-1], N, N + 2)
        _, nb_theirs = delta_bound(exact[-1], theirs[-1], N, 2 * N + 2)
        exact.append(nv), ours.append(nb_ours), theirs.append(nb_theirs)
    frame = lambda parts: torch.cat(parts, dim=1).transpose(1, 2).reshape(x.shape[0], -1)
    e, bo, bt = frame(exact), frame(ours), frame(theirs)
    err_f, err_c = (fused.double() - e).abs(), (composed.double() - fused.double()).abs()
    return (bool((err_f <= bo).all()) and bool((err_c <= bo + bt).all()),
            float((err_f / (bo + 1e-300)).max()), float((err_c / (bo + bt + 1e-300)).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--win-length", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "mfcc_time.jsonl"))
    args = ap.parse_args()
    be = default_backend()
    N = (args.win_length - 1) // 2

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    lines = []
    for n, n_clips in ((1 << 21, 2048), (17230, 10)):
        for n_mels, n_mfcc, orders in ((64, 13, 2), (64, 40, 2), (128, 40, 0)):
            g = torch.Generator(device=be.device).manual_seed(n_mels * 100 + n_mfcc)
            x = (torch.randn(n, n_mels, device=be.device, generator=g) * 18 - 35).contiguous()
            counts = [n // n_clips] * n_clips
            dct = be.from_host(be.dct_matrix(n_mfcc, n_mels))
            D = n_mfcc * (1 + orders)
            prefix, _ = be._frame_prefix(counts, n)
            out = be.empty((n, D))
            vp = lambda t: ctypes.c_void_p(t.data_ptr())

            def fused():
                return be.mfcc(x, counts, n_mfcc=n_mfcc, dct=dct, orders=orders, win_length=args.win_length)

            def native():
                _lib.check(be.lib.at_mfcc_f32(be.ctx.handle, vp(x), vp(prefix), n_clips, n, n_mels, n_mfcc, vp(dct), orders,
                                              args.win_length, 0, 0.0, vp(out), _lib.AT_LAYOUT_FRAME_MAJOR, be._stream()))

            def composed():
                return composition(x, dct, n_clips, orders, N)

            a, c = fused(), composed()
            native()
            ok, worst_f, worst_c = within_bound(x, dct, n_clips, orders, N, a, c)
            same_native = bool(torch.equal(a.view(torch.int32), out.view(torch.int32)))
            del a, c
            routes = {"fused": fused, "native": native, "composed": composed}
            for fn in routes.values():          # every shape warmed
                fn()
            times = {name: [] for name in routes}
            for _ in range(args.reps):
                for name, fn in routes.items():
                    times[name].append(timed(fn))
            med = {name: statistics.median(v) for name, v in times.items()}
            floor_ms = 4.0 * (n_mels + D) * n / (HBM_TBS * 1e12) * 1e3
            line = {"n_frames": n, "n_clips": n_clips, "n_mels": n_mels, "n_mfcc": n_mfcc, "orders": orders,
                    "win_length": args.win_length, "reps": args.reps, "what": "call times, host-synchronised, ms",
                    "within_test_bound": ok, "fused_error_over_bound": worst_f, "composed_minus_fused_over_bound": worst_c,
                    "native_bit_equal_fused": same_native,
                    **{f"{name}_ms": med[name] for name in routes},
                    **{f"{name}_ms_min_max": [min(times[name]), max(times[name])] for name in routes},
                    "composed_over_fused": med["composed"] / med["fused"],
                    "streaming_floor_ms": floor_ms, "floor_over_native": floor_ms / med["native"],
                    "kernel_trace": False, "device": torch.cuda.get_device_name(be.device)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del x, out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
