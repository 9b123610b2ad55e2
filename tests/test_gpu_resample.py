"""csrc/resample.hip, every kernel form at every rate pair, against tests/resample_ref.py: the exact model of the one
ascending-k fp32 fma chain per output sample that the file's header promises.

Every comparison is np.array_equal on bit patterns, with the float64 dot product and its analytic bound beside it; no
tolerance is guessed.  Inputs are views into NaN-filled device buffers (a read outside [0, L) shows in the bits),
outputs lie in buffers filled with a sentinel word with room behind every row (a store outside [0, out_len) shows
too).  The pairs sit on every branch of the drivers: the interleaved and the adjacent tile layout on both sides of
new = 32, the smallest tile and the first pair that no longer fits one, strong down- and up-sampling, and the rates real
data comes at; the lengths on every edge of a step and of a tile (resample_ref.lengths_for)."""
import ctypes

import numpy as np
import pytest
import torch

import resample_ref as R
from audio_tokens_amd import _lib

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 0x5A5A5A5A      # 1.5e16 as a float: no resampled test clip holds it
GUARD, PAD = 3, 5          # sentinel words in front of / behind the output buffer, and behind every output row
PAIRS = list(R.PAIRS)
CASES = [(o, n, L) for o, n in PAIRS for L in R.lengths_for(o, n)]
_vp = ctypes.c_void_p


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def nan_rows(be, w):
    """w [B, L] -> the rows as views into ONE NaN-filled device buffer: every row starts one float behind a 16-byte
    boundary and the row stride is 3 .. 6 floats above L."""
    B, L = w.shape
    stride = (L + 6) // 4 * 4
    buf = torch.full((1 + B * stride + 4,), NAN, device=be.device)
    v = buf[1: 1 + B * stride].view(B, stride)[:, :L]
    v.copy_(torch.from_numpy(np.array(w, dtype=np.float32)))      # (a copy: the shared references are read-only)
    assert v.data_ptr() % 16 == 4 and (B == 1 or v.stride(0) >= L + 3)
    return v


def resample_raw(be, v, orig_freq, new_freq, n_clips=None, L=None, wave_stride=None, out_stride=None):
    """at_resample_f32 as HipBackend.resample calls it, but into a sentinel-filled buffer with out_stride = out_len + PAD
    -> (return code, the whole buffer as uint32 on the host, out_len).  The keyword arguments override what the call
    is told about the buffers (argument checks)."""
    B, Lv = v.shape
    out_len = R.out_length(Lv, orig_freq, new_freq)
    stride = out_len + PAD
    buf = torch.full((GUARD + B * stride + GUARD,), SENTINEL, dtype=torch.int32, device=be.device)
    with torch.cuda.device(be.device):
        rc = be.lib.at_resample_f32(be.ctx.handle, _vp(v.data_ptr()), B if n_clips is None else n_clips,
                                    Lv if L is None else L, v.stride(0) if wave_stride is None else wave_stride, orig_freq,
                                    new_freq, _vp(buf.data_ptr() + 4 * GUARD), stride if out_stride is None else out_stride,
                                    be._stream())
    return rc, buf.cpu().numpy().view(np.uint32), out_len


def resample_guarded(be, v, orig_freq, new_freq):
    """-> the output rows' bits [B, out_len], after checking that every word around them still holds the sentinel."""
    rc, host, out_len = resample_raw(be, v, orig_freq, new_freq)
    _lib.check(rc)
    B, stride = v.shape[0], out_len + PAD
    body = host[GUARD: GUARD + B * stride].reshape(B, stride)
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + B * stride:] == SENTINEL).all(), "a store outside the buffer's rows"
    assert (body[:, out_len:] == SENTINEL).all(), \
        f"a store behind a row's out_len = {out_len}: columns {sorted(set(np.nonzero(body[:, out_len:] != SENTINEL)[1] + out_len))}"
    return body[:, :out_len]


def assert_bits(got, want, what):
    want = bits(want)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        b, o = bad[0]
        pytest.fail(f"{what}: {len(bad)} of {want.size} samples differ from the fma chain, first at row {b}, sample {o}: "
                    f"{got.view(np.float32)[b, o]!r} against {want.view(np.float32)[b, o]!r}")


@pytest.fixture()
def both_forms(switches):
    """The two settings of the test switch: the driver's own choice (tiled where the filter fits), and the plain
    one-thread-per-sample kernel whatever the pair."""
    def each():
        for simple in (0, 1):
            switches(resample_simple=simple)
            yield simple
    return each


# ---- the plan ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("orig_freq,new_freq", PAIRS)
def test_pair_table_is_what_the_plan_chooses(be, orig_freq, new_freq):
    """The branches this file means to reach are the ones the library takes: (orig, nw, width, K, mode, TI) of the
    group record at_frontend_plan_host writes, whose formulas at_resample_f32 repeats."""
    g = be.frontend_plan([1], [100], [orig_freq], new_freq, 64, 32)[2][0]
    R.check_plan_record(g, orig_freq, new_freq, _lib.AT_FRONTEND_TILED, _lib.AT_FRONTEND_SIMPLE)


# ---- every pair, every length, both kernels ------------------------------------------------------------------------------

@pytest.mark.parametrize("orig_freq,new_freq,L", CASES)
def test_kernels_are_the_fma_chain(be, both_forms, orig_freq, new_freq, L):
    w, want, val, bound = R.reference(orig_freq, new_freq, L)
    v = nan_rows(be, w)
    for simple in both_forms():
        got = resample_guarded(be, v, orig_freq, new_freq)
        assert_bits(got, want, f"{orig_freq} -> {new_freq}, L = {L}, resample_simple = {simple}")
        assert (np.abs(got.view(np.float32).astype(np.float64) - val) <= bound).all()


@pytest.mark.parametrize("orig_freq,new_freq", PAIRS)
def test_impulse_reads_out_the_tap_table(be, both_forms, orig_freq, new_freq):
    """A clip that is zero except x[p] = 1 resamples to the taps themselves (fma(0, t, acc) = acc, fma(1, t, +0) = t):
    output i*new + j is taps[j][p - i*orig + width], +0 elsewhere.  Pins the tap index, the window's start and the
    [K][new] transposition of the device table without the chain model."""
    orig, new, width = R.PAIRS[(orig_freq, new_freq)][:3]
    L = 3 * orig + width
    ps = sorted({p for p in (0, 1, width, L // 2, L - 1) if p < L})
    x = np.zeros((len(ps), L), np.float32)
    x[np.arange(len(ps)), ps] = 1.0
    want = np.stack([R.impulse_response(L, p, orig_freq, new_freq) for p in ps])
    v = nan_rows(be, x)
    for simple in both_forms():
        got = resample_guarded(be, v, orig_freq, new_freq)
        assert_bits(got, want, f"{orig_freq} -> {new_freq}, impulses at {ps}, resample_simple = {simple}")


# ---- the resident taps of at_resample_f32 --------------------------------------------------------------------------------

def test_single_slot_tap_cache_when_the_pair_alternates(be):
    """at_resample_f32 keeps ONE tap table resident: alternate between two pairs (of unequal table size, then of equal
    K), then change the key but not the reduced pair.  Every call must still be the chain of its own pair."""
    for A, B in (((44100, 22050, 8161), (48000, 22050, 7535)), ((11025, 22050, 8177), (8000, 48000, 8177))):
        va, vb = (nan_rows(be, R.reference(*c)[0]) for c in (A, B))
        for turn in range(2):
            for c, v in ((A, va), (B, vb)):
                assert_bits(resample_guarded(be, v, c[0], c[1]), R.reference(*c)[1], f"{c}, turn {turn}")
    w, want = R.reference(44100, 22050, 8161)[:2]
    v = nan_rows(be, w)
    assert_bits(resample_guarded(be, v, 44100, 22050), want, "44100 -> 22050")
    assert_bits(resample_guarded(be, v, 88200, 44100), want, "88200 -> 44100 behind 44100 -> 22050")
    assert_bits(resample_guarded(be, v, 44100, 22050), want, "44100 -> 22050 again")


# ---- argument checks -----------------------------------------------------------------------------------------------------

def refused(rc, match):
    assert rc < 0
    with pytest.raises(_lib.NativeError, match=match) as e:
        _lib.check(rc)
    assert e.value.code == rc


def test_argument_checks_and_the_largest_batch(be):
    rng = np.random.default_rng(65535)
    w = rng.standard_normal((65536, 1)).astype(np.float32)
    v = torch.from_numpy(w).to(be.device)
    # gridDim.y's limit: 65535 one-sample clips are one launch ...
    want = R.chain(w[:65535], 44100, 22050)
    assert_bits(resample_guarded(be, v[:65535], 44100, 22050), want, "65535 clips of one sample")
    # ... and one more is refused (HipBackend.resample cuts its batches there), with nothing written
    rc, host, _ = resample_raw(be, v, 44100, 22050)
    refused(rc, "at_resample_f32: bad arguments")
    assert (host == SENTINEL).all()

    w, want = R.reference(44100, 22050, 8161)[:2]
    v = nan_rows(be, w)
    rc, host, out_len = resample_raw(be, v, 44100, 22050, wave_stride=8160)
    refused(rc, "at_resample_f32: bad arguments")
    assert (host == SENTINEL).all()
    rc, host, out_len = resample_raw(be, v, 44100, 22050, out_stride=out_len - 1)
    refused(rc, f"out_stride < output length {out_len}")
    assert (host == SENTINEL).all()
    rc, host, _ = resample_raw(be, v, 44100, 22050, L=0)
    refused(rc, "at_resample_f32: bad arguments")
    # the context is none the worse for it
    assert_bits(resample_guarded(be, v, 44100, 22050), want, "44100 -> 22050 behind the refused calls")


# ---- the ragged form -----------------------------------------------------------------------------------------------------

FRONT = dict(n_fft=64, hop=32, n_mels=8)      # the log-mel half of frontend_ragged at its cheapest


def ragged_clip(C, L, seed):
    rng = np.random.default_rng([C, L, seed])
    x = 0.4 * np.sin(np.arange(L)[None, :] * (0.021 + 0.007 * np.arange(C)[:, None]) + seed)
    return (x + 0.1 * rng.standard_normal((C, L))).astype(np.float32)


def nan_packed(be, arrays):
    """The clips as views of ONE NaN-filled device buffer: 1 .. 3 floats of padding in front of each, stereo rows 5
    floats apart from their length; a clip of length 0 is an empty view."""
    total = sum(a.shape[0] * (a.shape[1] + 5) + 3 for a in arrays) + 8
    buf = torch.full((total,), NAN, device=be.device)
    views, pos = [], 0
    for i, a in enumerate(arrays):
        pos += 1 + i % 3
        C, L = a.shape
        v = buf[pos: pos + C * (L + 5)].view(C, L + 5)[:, :L]
        v.copy_(torch.from_numpy(a))
        views.append(v)
        pos += C * (L + 5)
    return views


_mono_ref = {}


def mono_chain(a, sr, common_sr):
    """The mono row of one clip: the chain of the clip, or of (l + r) * 0.5f in float32 for a stereo pair; once per
    clip."""
    key = (a.shape, sr, common_sr, a.tobytes())
    if key not in _mono_ref:
        m = a[0] if a.shape[0] == 1 else (a[0] + a[1]) * np.float32(0.5)
        _mono_ref[key] = R.chain(m, sr, common_sr) if m.size else np.zeros(0, np.float32)
    return _mono_ref[key]


def check_ragged(be, what, arrays, views, rates, common_sr):
    out, T, first, bad = be.frontend_ragged(views, rates, common_sr, pad_value=NAN, **FRONT)
    last = be.frontend_last
    mono = last["mono"].cpu().numpy()
    used = np.zeros(mono.size, bool)
    for i, (a, sr) in enumerate(zip(arrays, rates)):
        rec = last["plan"][i]
        want = mono_chain(a, sr, common_sr)
        assert rec["out_length"] == want.size == R.out_length(a.shape[1], sr, common_sr) and rec["mono_offset"] % 4 == 0
        row = mono[rec["mono_offset"]: rec["mono_offset"] + want.size]
        used[rec["mono_offset"]: rec["mono_offset"] + want.size] = True
        assert_bits(bits(row)[None], want[None], f"{what}: clip {i} (C = {a.shape[0]}, L = {a.shape[1]}, {sr} -> {common_sr})")
        assert T[i] == (0 if want.size <= FRONT["n_fft"] // 2 else be.num_frames(want.size, FRONT["hop"]))
    # the padding between the rows is still what it was filled with: nobody wrote across a boundary
    assert np.isnan(mono[~used]).all(), f"{what}: a store outside the mono rows"
    assert out.numel() == int(T.sum()) * FRONT["n_mels"] and not bad.cpu().numpy().any()
    return last


def test_ragged_more_rate_pairs_than_tap_slots(be):
    """Six resampled pairs in ONE batch against the four resident tap slots (replaced round robin): the fifth and sixth
    group evict the first two while the batch is still being queued, the repeat finds none of its pairs where it left
    them, a batch with a seventh pair moves the cursor, and the six come back.  Mono and stereo clips mixed, one clip
    per pair longer than a tile.  23 520 Hz is the lowest common rate all six reduced pairs exist at."""
    common = 23520
    six = [(47040, (2, 1)), (11760, (1, 2)), (70560, (3, 1)), (51200, (320, 147)), (21609, (147, 160)), (64827, (441, 160))]
    for sr, pair in six:
        assert R.reduced(sr, common) == pair
    lengths = {(2, 1): (8200, 301), (1, 2): (8190, 77), (3, 1): (8200, 55), (320, 147): (8001, 1500),
               (147, 160): (7800, 640), (441, 160): (7500, 2)}
    arrays, rates = [], []
    for n, (sr, pair) in enumerate(six):           # (clip order: the pairs interleaved, so no group is contiguous)
        arrays.append(ragged_clip(1 + n % 2, lengths[pair][0], n))
        rates.append(sr)
    for n, (sr, pair) in enumerate(six):
        arrays.append(ragged_clip(2 - n % 2, lengths[pair][1], 10 + n))
        rates.append(sr)
    views = nan_packed(be, arrays)
    seventh = [ragged_clip(2, 3001, 20), ragged_clip(1, 40, 21)]
    views7 = nan_packed(be, seventh)
    assert R.reduced(29400, common) == (5, 4)

    for turn in range(2):
        last = check_ragged(be, f"six pairs, call {turn}", arrays, views, rates, common)
        assert len(last["groups"]) == 6 and (last["groups"]["mode"] == _lib.AT_FRONTEND_TILED).all()
    check_ragged(be, "a seventh pair alone", seventh, views7, [29400, 29400], common)
    check_ragged(be, "six pairs behind the seventh", arrays, views, rates, common)
    # the slots belong to the context, not to a stream: the same on the background stream, once the main one is idle
    torch.cuda.synchronize()
    with torch.cuda.stream(be.background_stream()):
        check_ragged(be, "six pairs, background stream", arrays, views, rates, common)
        check_ragged(be, "the seventh pair, background stream", seventh, views7, [29400, 29400], common)
    torch.cuda.synchronize()
    check_ragged(be, "six pairs, main stream again", arrays, views, rates, common)


@pytest.mark.parametrize("sr,common,tiled", [(44100, 22050, True), (2045, 2044, False)])
def test_ragged_clips_without_blocks(be, sr, common, tiled):
    """Clips of length 0 own no workgroup and share their block prefix with the clip behind them: as the first, a
    middle (twice in a row) and the last member of a resampled group, among ordinary clips of one block and of
    several, the binary search of mix_resample_ragged_kernel must never land on one."""
    lengths = [0, 9000 if tiled else 3000, 0, 0, 300, 700, 0]
    chans = [1, 2, 2, 1, 1, 2, 2]
    arrays = [ragged_clip(C, L, 30 + i) for i, (C, L) in enumerate(zip(chans, lengths))]
    views = nan_packed(be, arrays)
    for turn in range(2):
        last = check_ragged(be, f"{sr} -> {common}, call {turn}", arrays, views, [sr] * len(arrays), common)
        g = last["groups"]
        assert len(g) == 1 and g[0]["mode"] == (_lib.AT_FRONTEND_TILED if tiled else _lib.AT_FRONTEND_SIMPLE)
        assert g[0]["n_blocks"] > 3          # (the long clip alone has several)
        for i, L in enumerate(lengths):
            if L == 0:
                assert last["plan"][i]["out_length"] == 0 and last["plan"][i]["n_frames"] == 0
