"""ops.MFCC / ops.ComputeDeltas / at_mfcc_f32 / at_deltas_f32 on the MI355X, bit for bit against tests/mfcc_ref.py
(NaN positions equal), on synthetic rows fed straight to HipBackend.mfcc so that clip geometry is free; then from
audio, against the model applied to the device's own log-mel output and against the restated torchaudio composition
within a bound computed from the data."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mfcc_ref as R

pytestmark = pytest.mark.gpu

TB = R.TB
SHAPES = [(64, 13), (64, 40), (64, 64), (128, 40), (40, 40), (23, 13), (64, 1)]


def _np(t):
    return t.detach().cpu().numpy()


def rows_like_db(n, n_mels, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, n_mels)) * 18 - 35).astype(np.float32)


def geometry(N):
    """Every clip length of the issue and the ragged arrangements, in one batch: empty clips at the start, in the
    middle, in runs and at the end; clips that end exactly on a tile edge; one clip of several tiles between clips of
    one frame."""
    counts = [0, 1, 2, 3, 2 * N, 2 * N + 1, 4 * N + 1, 0, TB - 1, TB, TB + 1, 2 * TB + 3, 0, 0, 0]
    counts.append(TB - sum(counts) % TB)          # ... the next clips start and end on tile edges
    counts += [TB, 2 * TB, 1, 3 * TB + 8, 1, 0, 0]
    return counts


@functools.lru_cache(maxsize=None)
def case(n_mels, n_mfcc, win_length):
    """-> (x, counts, table, {orders: frame-major reference}), computed once and shared by the layouts and orders."""
    counts = geometry((win_length - 1) // 2)
    x = rows_like_db(sum(counts), n_mels, 1000 * n_mels + 10 * n_mfcc + win_length)
    table = R.dct_table(n_mfcc, n_mels)
    full = R.mfcc_ref(x, counts, table, orders=2, win_length=win_length)
    return x, counts, table, {o: np.ascontiguousarray(full[:, :n_mfcc * (1 + o)]) for o in (0, 1, 2)}


def check(got, ref, counts, frame_major, what):
    want = ref if frame_major else R.feature_major(ref, counts)
    got = _np(got)
    assert got.shape == want.shape, what
    if not R.same_bits(got, want):
        bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ, first at {bad[:5]}")


@pytest.mark.parametrize("frame_major", [True, False], ids=["frame_major", "feature_major"])
@pytest.mark.parametrize("win_length", [3, 5, 9])
@pytest.mark.parametrize("orders", [0, 1, 2])
@pytest.mark.parametrize("n_mels,n_mfcc", SHAPES)
def test_mfcc_every_shape_order_window_and_layout(be, n_mels, n_mfcc, orders, win_length, frame_major):
    x, counts, table, ref = case(n_mels, n_mfcc, win_length)
    assert np.array_equal(be.dct_matrix(n_mfcc, n_mels), table)
    got = be.mfcc(x, counts, n_mfcc=n_mfcc, orders=orders, win_length=win_length, frame_major=frame_major)
    check(got, ref[orders], counts, frame_major, (n_mels, n_mfcc, orders, win_length))


@pytest.mark.parametrize("n_mels,n_mfcc,win_length,counts", [
    (128, 128, 9, [0, 70, 1, 200, 0, 3]),        # the table does not fit beside the tile: read through L2
    (320, 320, 5, [40, 0, 1, 90]),               # ... and the coefficients split over two blocks in y
    (1024, 8, 5, [5, 16, 0, 43, 1]),             # rows too wide for a tile of 64 frames
])
def test_mfcc_wide_rows_take_the_other_forms(be, n_mels, n_mfcc, win_length, counts):
    x = rows_like_db(sum(counts), n_mels, n_mels + n_mfcc)
    table = R.dct_table(n_mfcc, n_mels)
    ref = R.mfcc_ref(x, counts, table, orders=2, win_length=win_length, top_db=60.0)
    for frame_major in (True, False):
        got = be.mfcc(x, counts, n_mfcc=n_mfcc, orders=2, win_length=win_length, top_db=60.0, frame_major=frame_major)
        check(got, ref, counts, frame_major, (n_mels, n_mfcc, frame_major))


@pytest.mark.parametrize("n_mels,n_mfcc", [(64, 40), (64, 13), (23, 13)])
def test_top_db_is_per_clip(be, n_mels, n_mfcc):
    counts = [0, 30, 50, TB, 0, 2 * TB + 5, 1, 7]
    x = rows_like_db(sum(counts), n_mels, 5 + n_mfcc)
    first = R.prefix_of(counts)
    x[first[1]:first[2]] = x[first[1]:first[2]] * 0.2 - 20
    x[first[2] - 1, n_mels // 3] = 55.0                    # the maximum sits in the clip's last frame
    x[first[2]:first[3]] = x[first[2]:first[3]] * 0.1 - 190    # entirely below the floor of both neighbours
    x[first[5] + TB, 0] = 40.0
    table = R.dct_table(n_mfcc, n_mels)
    for top_db in (None, 80.0, 30.0, 0.0):
        ref = R.mfcc_ref(x, counts, table, orders=2, win_length=5, top_db=top_db)
        for frame_major in (True, False):
            got = be.mfcc(x, counts, n_mfcc=n_mfcc, orders=2, win_length=5, top_db=top_db, frame_major=frame_major)
            check(got, ref, counts, frame_major, (n_mfcc, top_db, frame_major))
    quiet = R.mfcc_ref(x[first[2]:first[3]], [counts[2]], table, top_db=30.0)
    both = _np(be.mfcc(x, counts, n_mfcc=n_mfcc, top_db=30.0))
    assert R.same_bits(both[first[2]:first[3]], quiet)      # the quiet clip did not see its neighbours' floors
    assert not R.same_bits(quiet, R.mfcc_ref(np.maximum(x[first[2]:first[3]], np.float32(25.0)), [counts[2]], table))


@pytest.mark.parametrize("orders,win_length", [(2, 5), (2, 9), (1, 3)])
def test_non_finite_frames_reach_orders_times_n_frames_and_no_other_clip(be, orders, win_length):
    n_mels, n_mfcc, N = 64, 40, (win_length - 1) // 2
    counts = [TB - 3, 2 * TB + 9, 40]
    x = rows_like_db(sum(counts), n_mels, 77)
    table = R.dct_table(n_mfcc, n_mels)
    clean = R.mfcc_ref(x, counts, table, orders=orders, win_length=win_length)
    s = counts[0]
    for value, at in [(np.nan, s + 70), (np.inf, s + 63), (-np.inf, s + 64), (np.nan, s), (np.inf, s + counts[1] - 1)]:
        y = x.copy()
        y[at, 5] = value
        ref = R.mfcc_ref(y, counts, table, orders=orders, win_length=win_length)
        got = _np(be.mfcc(y, counts, n_mfcc=n_mfcc, orders=orders, win_length=win_length))
        assert R.same_bits(got, ref), (value, at)
        reach = orders * N
        lo, hi = max(at - reach, s), min(at + reach, s + counts[1] - 1)
        assert not np.isfinite(got[at, :n_mfcc]).any()                   # the frame's own coefficients
        untouched = np.r_[0:lo, hi + 1:sum(counts)]                      # the stated reach, and nothing beyond, in any clip
        assert np.array_equal(got[untouched].view(np.uint32), clean[untouched].view(np.uint32)), (value, at)
        # under top_db the whole clip is NaN (a NaN) and the neighbours are untouched bit for bit
        ref = R.mfcc_ref(y, counts, table, orders=orders, win_length=win_length, top_db=80.0)
        got = _np(be.mfcc(y, counts, n_mfcc=n_mfcc, orders=orders, win_length=win_length, top_db=80.0))
        assert R.same_bits(got, ref), (value, at)
        if value != value:
            assert np.isnan(got[s:s + counts[1]]).all() and np.isfinite(got[:s]).all() and np.isfinite(got[s + counts[1]:]).all()


def test_constant_clips_and_single_frames_give_exact_zero_deltas(be):
    counts = [1, 2 * TB + 1, 1, 1, 9]
    x = rows_like_db(sum(counts), 64, 9)
    x[1:2 * TB + 2] = x[1]
    for win_length in (3, 5, 9):
        got = be.mfcc(x, counts, n_mfcc=13, orders=2, win_length=win_length)
        check(got, R.mfcc_ref(x, counts, R.dct_table(13, 64), 2, win_length), counts, True, win_length)
        assert not _np(got)[:2 * TB + 4, 13:].view(np.uint32).any()
    assert _np(got)[2 * TB + 4:, 13:].view(np.uint32).any()


def test_a_callers_own_table_and_the_unnormalised_one(be):
    counts = [3, TB + 2, 0, 20]
    x = rows_like_db(sum(counts), 40, 11)
    own = np.random.default_rng(12).standard_normal((40, 17)).astype(np.float32)
    got = be.mfcc(x, counts, n_mfcc=17, dct=own, orders=2, win_length=5, top_db=70.0)
    check(got, R.mfcc_ref(x, counts, own, 2, 5, 70.0), counts, True, "own table")
    got = be.mfcc(x, counts, n_mfcc=17, norm=None, orders=1)
    check(got, R.mfcc_ref(x, counts, R.dct_table(17, 40, ortho=False), 1, 5), counts, True, "norm=None")
    torch_table = R.create_dct_torch(17, 40).numpy()
    got = be.mfcc(x, counts, n_mfcc=17, dct=torch_table)
    check(got, R.mfcc_ref(x, counts, torch_table), counts, True, "torchaudio's table")
    with pytest.raises(ValueError):
        be.mfcc(x, counts, n_mfcc=17, dct=own.T.copy())
    with pytest.raises(ValueError):
        be.mfcc(x, [3, 4], n_mfcc=17)


def test_pointers_offset_by_one_float(be):
    """Rows and output that are not 16-byte aligned take the scalar loads and stores."""
    x, counts, table, ref = case(64, 40, 5)
    n = x.shape[0]
    xin = be.empty((n * 64 + 1,))[1:].view(n, 64)
    xin.copy_(torch.from_numpy(x))
    out = be.empty((n * 120 + 1,))[1:].view(n, 120)
    assert xin.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    got = be.mfcc(xin, counts, n_mfcc=40, orders=2, out=out)
    assert got.data_ptr() == out.data_ptr()
    check(got, ref[2], counts, True, "offset rows and output")
    check(be.mfcc(x, counts, n_mfcc=40, orders=2, out=out), ref[2], counts, True, "offset output")
    d = be.empty((n * 64 + 1,))[1:].view(n, 64)
    check(be.deltas(xin, counts, out=d), R.deltas_ref(x, counts, 5), counts, True, "offset deltas")


def test_argument_errors_and_empty_calls_through_the_c_abi(be):
    lib, h, null = be.lib, be.ctx.handle, ctypes.c_void_p(None)
    x = be.zeros((8, 64))
    first = torch.tensor([0, 8], dtype=torch.int64, device=be.device)
    out = be.zeros((8, 120))
    table = be.from_host(R.dct_table(40, 64))
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def mfcc(ctx=h, x=p(x), first=p(first), n_clips=1, n=8, n_mels=64, n_mfcc=40, dct=p(table), orders=2, win=5, use=0,
             top=0.0, out=p(out), layout=1):
        return lib.at_mfcc_f32(ctx, x, first, n_clips, n, n_mels, n_mfcc, dct, orders, win, use, top, out, layout, null)

    assert mfcc() == 0 and mfcc(dct=null) == 0 and mfcc(use=1, top=80.0, layout=0) == 0
    for bad in [dict(ctx=null), dict(x=null), dict(first=null), dict(out=null), dict(win=4), dict(win=1), dict(win=-3),
                dict(orders=3), dict(orders=-1), dict(n_mfcc=0), dict(n_mfcc=65), dict(n_mels=0), dict(n_mels=1025, n_mfcc=1),
                dict(use=1, top=-1.0), dict(use=1, top=float("nan")), dict(layout=2), dict(n=-1), dict(n_clips=-1),
                dict(n_mels=1024, n_mfcc=8, win=65)]:
        assert mfcc(**bad) == -1, bad
        assert b"at_mfcc_f32" in lib.at_last_error(), bad
    assert mfcc(use=0, top=-1.0) == 0                       # an unused top_db is not looked at
    assert mfcc(n=0, x=null, out=null) == 0 and mfcc(n_clips=0, first=null) == 0     # nothing to do: no pointer is touched

    def deltas(ctx=h, x=p(x), first=p(first), n_clips=1, n=8, F=64, win=5, out=p(out)):
        return lib.at_deltas_f32(ctx, x, first, n_clips, n, F, win, out, null)

    assert deltas() == 0
    for bad in [dict(ctx=null), dict(x=null), dict(first=null), dict(out=null), dict(win=2), dict(win=1), dict(F=0),
                dict(n=-1)]:
        assert deltas(**bad) == -1, bad
        assert b"at_deltas_f32" in lib.at_last_error(), bad
    assert deltas(n=0, x=null) == 0 and deltas(n_clips=0, first=null) == 0
    be.synchronize()
    # the library's own table (dct = null) is the one of at_dct_matrix_host
    xr = rows_like_db(8, 64, 1)
    x.copy_(torch.from_numpy(xr))
    assert mfcc(dct=null) == 0
    assert R.same_bits(_np(out), R.mfcc_ref(xr, [8], R.dct_table(40, 64), 2, 5))
    # n = 0 through the Python layer
    assert tuple(be.mfcc(be.zeros((0, 64)), [0, 0], n_mfcc=13, orders=2).shape) == (0, 39)
    assert tuple(be.mfcc(be.zeros((0, 64)), [], n_mfcc=13, frame_major=False).shape) == (0,)
    assert tuple(be.deltas(be.zeros((0, 5)), [0]).shape) == (0, 5)


def test_two_streams_at_once_with_different_tables(be):
    x1, c1, t1, r1 = case(64, 40, 5)
    x2, c2, t2, r2 = case(128, 40, 9)
    ref1 = R.mfcc_ref(x1, c1, t1, 2, 5, top_db=50.0)
    own = np.random.default_rng(3).standard_normal((128, 40)).astype(np.float32)
    ref2 = R.mfcc_ref(x2, c2, own, 2, 9, top_db=20.0)
    d1, d2, o2 = be.from_host(x1), be.from_host(x2), be.from_host(own)
    be.synchronize()
    s1, s2 = torch.cuda.Stream(device=be.device), torch.cuda.Stream(device=be.device)
    got = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            a = be.mfcc(d1, c1, n_mfcc=40, orders=2, win_length=5, top_db=50.0)
        with torch.cuda.stream(s2):
            b = be.mfcc(d2, c2, n_mfcc=40, dct=o2, orders=2, win_length=9, top_db=20.0, frame_major=False)
        got.append((a, b))
    s1.synchronize()
    s2.synchronize()
    for a, b in got:
        check(a, ref1, c1, True, "stream 1")
        check(b, ref2, c2, False, "stream 2")


@pytest.mark.parametrize("F", [1, 13, 64, 700])
@pytest.mark.parametrize("win_length", [3, 5, 9])
def test_deltas_alone(be, F, win_length):
    from audio_tokens_amd import ops
    counts = geometry((win_length - 1) // 2) if F <= 64 else [0, 3, 70, 1]
    c = rows_like_db(sum(counts), F, F + win_length)
    got = be.deltas(c, counts, win_length=win_length)
    check(got, R.deltas_ref(c, counts, win_length), counts, True, (F, win_length))
    # ops.ComputeDeltas on [B, F, T]
    B, T = 3, TB + 5
    spec = rows_like_db(B * T, F, 2 * F + win_length).reshape(B, T, F).transpose(0, 2, 1).copy()
    out = ops.ComputeDeltas(win_length, backend=be)(torch.from_numpy(spec))
    want = R.deltas_ref(spec.transpose(0, 2, 1).reshape(B * T, F), [T] * B, win_length).reshape(B, T, F).transpose(0, 2, 1)
    assert tuple(out.shape) == (B, F, T) and out.device.type == "cuda" and out.is_contiguous()
    assert R.same_bits(_np(out), np.ascontiguousarray(want))
    assert R.same_bits(_np(ops.ComputeDeltas(win_length, backend=be)(torch.from_numpy(spec[0]))), np.ascontiguousarray(want[0]))


# ---- from audio ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def audio():
    from audio_tokens_amd.synth import synth_clips
    return synth_clips(4, L=9000, seed=99, device="cpu")


def test_ops_mfcc_from_audio_is_the_model_on_the_devices_own_logmel(be):
    from audio_tokens_amd import ops
    wave = audio()
    logmel = ops.LogMelSpectrogram(backend=be)
    rows = _np(logmel.frames(wave))
    T = rows.shape[0] // 4
    for kw in [dict(), dict(n_mfcc=13, deltas=2), dict(n_mfcc=13, deltas=2, top_db=None, win_length=9),
               dict(top_db=None, deltas=0, norm=None)]:
        m = ops.MFCC(backend=be, **kw)
        table = R.dct_table(m.n_mfcc, 64, ortho=m.norm == "ortho")
        ref = R.mfcc_ref(rows, [T] * 4, table, m.deltas, m.win_length, m.top_db)
        assert R.same_bits(_np(m.frames(wave)), ref), kw
        out = m(wave.reshape(2, 2, -1))
        assert tuple(out.shape) == (2, 2, m.D, T)
        assert R.same_bits(_np(out).reshape(4, m.D, T), np.ascontiguousarray(ref.reshape(4, T, m.D).transpose(0, 2, 1))), kw
        unit = _np(m.frames(wave, l2norm=True))
        assert R.same_bits(unit, _np(be.l2norm_rows(be.from_host(ref)))), kw
    # top_db=None, deltas=0: the DCT of exactly what LogMelSpectrogram returns
    spec = _np(logmel(wave))                                               # [4, 64, T]
    m = ops.MFCC(top_db=None, backend=be)
    want = R.coefficients_ref(spec.transpose(0, 2, 1).reshape(-1, 64), R.dct_table(40, 64))
    assert R.same_bits(_np(m.frames(wave)), want)


def test_ops_mfcc_batch_mixed_rates_stereo_and_a_short_clip(be):
    from audio_tokens_amd import ops
    wave = audio()
    rng = np.random.default_rng(5)
    clips = [wave[0], torch.from_numpy(rng.standard_normal((2, 7000)).astype(np.float32) * 0.1), wave[1][:100],
             wave[2][:16000 // 3], wave[3]]
    rates = [22050, 44100, 22050, 16000, 22050]
    m = ops.MFCC(n_mfcc=13, deltas=2, backend=be)
    got = m.batch(clips, rates)
    specs = ops.LogMelSpectrogram(backend=be).batch(clips, rates)
    assert got[2] is None and specs[2] is None and not _np(m.last_bad).any()
    counts = [0 if s is None else s.shape[1] for s in specs]
    rows = np.concatenate([_np(s).T for s in specs if s is not None])
    ref = R.mfcc_ref(rows, counts, R.dct_table(13, 64), 2, 5, 80.0)
    first = R.prefix_of(counts)
    for i, g in enumerate(got):
        if g is not None:
            assert tuple(g.shape) == (39, counts[i])
            assert R.same_bits(_np(g), np.ascontiguousarray(ref[first[i]:first[i + 1]].T)), i


def test_default_form_against_the_torchaudio_composition(be):
    """ops.MFCC's defaults (top_db = 80) with two delta orders against amplitude_to_DB's clamp, matmul with create_dct
    and compute_deltas twice, restated and run by torch on the CPU, clip by clip, on the device's own log-mel.  The bound
    comes from the data: gamma_64 * sum |x| |dct| for either chain plus sum |x| |dct - dct_torch| for the table, carried
    through the two delta stages with their own roundings (mfcc_ref.delta_exact_and_bound)."""
    from audio_tokens_amd import ops
    wave = audio()
    rows = _np(ops.LogMelSpectrogram(backend=be).frames(wave))
    T = rows.shape[0] // 4
    counts = [T] * 4
    got = _np(ops.MFCC(deltas=2, backend=be).frames(wave)).astype(np.float64)
    t_torch = R.create_dct_torch(40, 64)
    want = []
    for i in range(4):
        spec = R.amplitude_to_db_clamp_torch(torch.from_numpy(rows[i * T:(i + 1) * T].T.copy()), 80.0)     # [64, T]
        c = torch.matmul(spec.transpose(-1, -2), t_torch).transpose(-1, -2)
        d = R.compute_deltas_torch(c)
        want.append(torch.cat([c, d, R.compute_deltas_torch(d)], dim=0).numpy().T)
    want = np.concatenate(want).astype(np.float64)
    table = R.dct_table(40, 64).astype(np.float64)
    x = R.top_db_ref(rows, counts, 80.0).astype(np.float64)                 # (the clamp is exact in both)
    ax = np.abs(x)
    v0 = x @ table
    b_ours = R.gamma(64) * (ax @ np.abs(table))
    b_torch = R.gamma(64) * (ax @ np.abs(t_torch.numpy().astype(np.float64))) + ax @ np.abs(table - t_torch.numpy())
    v1, b1_ours = R.delta_exact_and_bound(v0, b_ours, counts, 5, 4)
    _, b1_torch = R.delta_exact_and_bound(v0, b_torch, counts, 5, 6)
    v2, b2_ours = R.delta_exact_and_bound(v1, b1_ours, counts, 5, 4)
    _, b2_torch = R.delta_exact_and_bound(v1, b1_torch, counts, 5, 6)
    exact = np.concatenate([v0, v1, v2], axis=1)
    ours = np.concatenate([b_ours, b1_ours, b2_ours], axis=1)
    both = ours + np.concatenate([b_torch, b1_torch, b2_torch], axis=1)
    for name, err, bound in [("device - exact", np.abs(got - exact), ours), ("device - torch", np.abs(got - want), both)]:
        print(f"{name}: max error {err.max():.3e}, max error / bound {(err / (bound + 1e-300)).max():.3f}")
        assert (err <= bound).all(), name


def test_audio_tokenizer_from_features(be):
    """12 ragged clips, 40 x 3 features, a 256-word vocabulary: the tokens are IndexFlatL2.search on
    l2norm_rows(mfcc(...)) composed by hand; a flagged clip gives None."""
    from audio_tokens_amd import ops
    from audio_tokens_amd.synth import synth_clips
    lens = [3000, 5000, 4100, 9000, 2000, 100, 7777, 6000, 3333, 8000, 4500, 5120]
    wave = synth_clips(12, L=9000, seed=7, device="cpu")
    clips = [wave[i][:L].clone() for i, L in enumerate(lens)]
    clips[4][1000] = float("nan")
    feats = ops.MFCC(n_mfcc=40, deltas=2, backend=be)
    vocab = np.random.default_rng(8).standard_normal((256, 120)).astype(np.float32)
    vocab /= np.linalg.norm(vocab, axis=1, keepdims=True)
    tok = ops.AudioTokenizer.from_features(vocab, feats, backend=be)
    tokens = tok.encode(clips)
    assert tokens[4] is None and tokens[5] is None              # flagged; too short
    rows, T, first, bad = be.frontend_ragged(clips, 22050, 22050, 512, 128, 64, frame_major=True, l2norm=False)
    assert _np(bad)[4] != 0 and T[5] == 0
    unit = be.l2norm_rows(be.mfcc(rows, T, n_mfcc=40, orders=2, win_length=5, top_db=80.0))
    index = ops.IndexFlatL2(120, backend=be)
    index.add(vocab)
    _, ids = index.search(unit, 1)
    ids = np.asarray(_np(ids) if isinstance(ids, torch.Tensor) else ids).reshape(-1)
    for i in range(12):
        if i in (4, 5):
            continue
        assert tokens[i].dtype == torch.int64 and np.array_equal(tokens[i].numpy(), ids[first[i]:first[i] + T[i]]), i
    with pytest.raises(AssertionError):
        ops.AudioTokenizer.from_features(vocab[:, :64].copy(), feats, backend=be)      # the vocabulary must be [k, D]
    # the default path is untouched
    plain = ops.AudioTokenizer(vocab[:, :64].copy(), backend=be)
    assert plain.features is None and plain.encode(clips[:2])[0].shape[0] == T[0]


def test_large_ragged_call_against_the_same_kernel_clip_by_clip(be):
    """2^18 frames in 300 uneven clips at (64, 40, orders 2): every clip run alone gives the same bits."""
    rng = np.random.default_rng(2718)
    n = 1 << 18
    cuts = np.sort(rng.choice(np.arange(1, n), size=299, replace=False))
    counts = np.diff(np.r_[0, cuts, n])
    counts[[5, 100]] += counts[[6, 101]]
    counts[[6, 101]] = 0
    assert counts.sum() == n and len(counts) == 300
    g = torch.Generator(device="cpu").manual_seed(1)
    x = (torch.randn((n, 64), generator=g) * 18 - 35).to(be.device)
    whole = be.mfcc(x, counts, n_mfcc=40, orders=2, win_length=5, top_db=80.0)
    first = R.prefix_of(counts)
    alone = be.empty((n, 120))
    for i in range(300):
        if counts[i]:
            be.mfcc(x[first[i]:first[i + 1]], [counts[i]], n_mfcc=40, orders=2, win_length=5, top_db=80.0,
                    out=alone[first[i]:first[i + 1]])
    assert torch.equal(whole.view(torch.int32), alone.view(torch.int32))
    # and a sample of it against the model
    i = int(np.argmax(counts > 200))
    ref = R.mfcc_ref(_np(x[first[i]:first[i + 1]]), [counts[i]], R.dct_table(40, 64), 2, 5, 80.0)
    assert R.same_bits(_np(whole[first[i]:first[i + 1]]), ref)
