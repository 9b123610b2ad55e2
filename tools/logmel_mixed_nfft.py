"""Times at_logmel_f32 at the even transform sizes that are not powers of two (development aid; the figures of DESIGN.md
section 5.0b and profiles/logmel_mixed_nfft.txt): per size, at hop = n_fft/2 and 64 mels over 5000 ten-second clips, the
mixed-radix form, the Bluestein form forced on the same size (switch logmel_fallback), the next power of two above, and
the torch composition on the device (torch.stft + matmul + log10, fp32).

The native configurations share one table slot per context (WS_LOGMEL_ANY: window, twiddles, filterbank, chirp tables),
so the first call after a change of (n_fft, form) rebuilds the tables on the host and synchronises the device.  A
round therefore takes the four configurations in turn, and for each makes one untimed call (tables resident again) and
then times `--calls` back-to-back calls between two events; the per-call time of a group is one sample, the median
over the rounds is reported.

    python tools/logmel_mixed_nfft.py [--rounds 7] [--calls 3] [--clips 5000] [n_fft ...]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from audio_tokens_amd.backend import default_backend

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--clips", type=int, default=5000)
ap.add_argument("sizes", nargs="*", type=int, default=[400, 480, 640, 882, 1000, 2000, 4000, 2038, 4094])
args = ap.parse_args()

be = default_backend()
SR, N_MELS, L = 22050, 64, 220500
g = torch.Generator(device="cuda").manual_seed(0)
w = torch.rand(args.clips, L, device="cuda", generator=g) * 0.2 - 0.1


def timed(fn):
    """ms per call of `args.calls` back-to-back calls, behind one untimed call of the same configuration"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / args.calls


def native(n_fft, fallback):
    T = be.num_frames(L, n_fft // 2)
    out = be.empty((args.clips * T, N_MELS))          # (no allocation inside the timed calls)

    def run():
        be.debug_set("logmel_fallback", fallback)
        be.logmel(w, SR, n_fft, n_fft // 2, N_MELS, frame_major=True, out=out)
    return run


def torch_composition(n_fft):
    fb = torch.from_numpy(be.mel_filterbank(SR, n_fft, N_MELS)).cuda()
    win = torch.hann_window(n_fft, periodic=True, device="cuda")

    def run():
        st = torch.stft(w, n_fft, n_fft // 2, window=win, center=True, pad_mode="reflect", return_complex=True)
        p = st.real ** 2 + st.imag ** 2
        mel = p.transpose(1, 2) @ fb
        return 10.0 * torch.log10(torch.clamp(mel, min=1e-10))
    return run


print(f"{args.clips} clips of {L} samples, hop = n_fft/2, {N_MELS} mels, frame-major; median over {args.rounds} rounds of "
      f"the per-call time of {args.calls} back-to-back calls, the four configurations in turn within a round", flush=True)
for n_fft in args.sizes:
    pow2 = 1 << (n_fft - 1).bit_length()
    hop = n_fft // 2
    frames = args.clips * (1 + L // hop)
    be.debug_set("logmel_fallback", 0)
    runs = {"native": native(n_fft, 0), "bluestein": native(n_fft, 1), f"pow2 {pow2}": native(pow2, 0),
            "torch": torch_composition(n_fft)}
    for fn in runs.values():                          # warm-up: allocator, FFT plans
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    be.debug_set("logmel_fallback", 0)
    med = {k: statistics.median(v) for k, v in ms.items()}
    frames2 = args.clips * (1 + L // (pow2 // 2))
    tbs = frames * (hop * 4 + N_MELS * 4) / med["native"] / 1e9
    tbs2 = frames2 * (pow2 // 2 * 4 + N_MELS * 4) / med[f"pow2 {pow2}"] / 1e9
    tbs_b = frames * (hop * 4 + N_MELS * 4) / med["bluestein"] / 1e9
    print(f"n_fft={n_fft:5d} frames={frames:8d}  native {med['native']:8.3f} ms ({med['native'] / frames * 1e6:6.2f} ns/frame, "
          f"{tbs:5.2f} TB/s algorithmic)  bluestein {med['bluestein']:8.3f} ms ({tbs_b:5.2f} TB/s)  pow2 {pow2}: {med[f'pow2 {pow2}']:8.3f} ms "
          f"({med[f'pow2 {pow2}'] / frames2 * 1e6:6.2f} ns/frame over {frames2} frames, {tbs2:5.2f} TB/s)  torch {med['torch']:8.3f} ms  "
          f"[min/max native {min(ms['native']):.3f}/{max(ms['native']):.3f}]", flush=True)
