"""ops.ResidualQuantizer(max_beam_size=B) / at_rq_beam_step_f32 / at_rq_beam_encode_f32 on the MI355X, bit for bit
against tests/rq_beam_ref.py (tests/knn_ref.py over the residuals of all beams, one lexsort per row on (D, parent slot,
word), numpy float32 subtraction)."""
import ctypes

import numpy as np
import pytest
import torch

from rq_beam_ref import beam_widths, partial_fill_case, path_tie_case, rq_beam_encode_ref, rq_beam_step_ref
from rq_ref import rq_encode_ref

pytestmark = pytest.mark.gpu

# (d, M, B): the fused top-k sweep with x in registers (d = 64, 128), B = 32: its widest list, B = 1: the greedy rule;
# d = 8, 12: the any-d sweep; d = 50: scalar lists and the scalar select kernel (d % 4 != 0); d = 640: ten chunks
SHAPES = [(64, 3, 5), (64, 2, 32), (128, 2, 4), (64, 4, 1), (8, 3, 3), (12, 2, 5), (50, 2, 2), (640, 2, 2)]
# B = 5: n = 3 is 15 beam rows behind stage 0 (direct form throughout), n = 4 is 20 (the form changes between stage 0
# and stage 1), n = 19 changes it at stage 1 for every B > 1; 33, 129: past a select workgroup (8 rows), a sweep tile
NS = [1, 3, 4, 19, 20, 33, 129, 1031]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _check(got, ref, label=""):
    """got: (codes, dist, residual, bad) of be.rq_beam_encode; ref: rq_beam_encode_ref's."""
    codes, dist, res, bad = _np(got[0]), _np(got[1]), _np(got[2]), int(got[3].item())
    cr, dr, rr, br = ref
    assert codes.dtype == np.uint8 and codes.shape == cr.shape and dist.shape == dr.shape and res.shape == rr.shape, label
    wrong = np.argwhere((codes != cr) | (bits(dist) != bits(dr)))
    assert wrong.size == 0, (label, wrong[:5], codes[wrong[0][0]], cr[wrong[0][0]], dist[wrong[0][0]], dr[wrong[0][0]])
    wrong = np.argwhere(bits(res) != bits(rr))
    assert wrong.size == 0, (label, "residual", wrong[:5], res[tuple(wrong[0])], rr[tuple(wrong[0])])
    assert bad == int(br), label


def _check_step(got, ref, label=""):
    """got: (r_out, parent, code, dist, bad) of be.rq_beam_step; ref: rq_beam_step_ref's."""
    for name, g, r in zip(("r_out", "parent", "code", "dist"), got[:4], ref[:4]):
        g = _np(g)
        assert g.dtype == r.dtype and g.shape == r.shape, (label, name, g.dtype, g.shape, r.shape)
        wrong = np.argwhere(g.view(np.uint8) != r.view(np.uint8))
        assert wrong.size == 0, (label, name, wrong[:5], g[tuple(wrong[0][:2])], r[tuple(wrong[0][:2])])
    assert int(got[4].item()) == int(ref[4]), label


def _data(seed, n, d, M, ksub=256):
    """Codebooks that get finer stage by stage, and rows near sums of one word per stage."""
    rng = np.random.default_rng(seed)
    cb = rng.standard_normal((M, ksub, d)).astype(np.float32)
    for m in range(M):
        cb[m] *= np.float32(0.5 ** m)
    x = rng.standard_normal((n, d)).astype(np.float32)
    if n > 3:
        q = 3 * n // 4
        pick = rng.integers(0, ksub, (q, M))
        near = np.zeros((q, d), np.float32)
        for m in range(M):
            near = near + cb[m][pick[:, m]]
        x[:q] = (near + np.float32(0.5 ** M * 0.3) * x[:q]).astype(np.float32)
    return x, cb


@pytest.mark.parametrize("d,M,B", SHAPES)
def test_beam_encode_grid_bit_exact(be, oracle, d, M, B):
    xall, cb = _data(d * 31 + M + B, max(NS), d, M)
    cbd = be._f32(cb)
    full = rq_beam_encode_ref(oracle, xall, cb, B)     # rows are independent: a call of n >= 20 rows is a prefix of it
    assert not full[3]
    for n in NS:
        x = xall[:n]
        ref = rq_beam_encode_ref(oracle, x, cb, B) if n < 20 else (full[0][:n], full[1][:n], full[2][:n], False)
        _check(be.rq_beam_encode(x, cbd, B, want_dist=True, want_residual=True), ref, (d, M, B, n))
        if B == 1:
            greedy = be.rq_encode(x, cbd, want_dist=True, want_residual=True)
            _check(greedy, ref, ("rq_encode", n))
    if B > 1:
        greedy = rq_encode_ref(oracle, xall, cb)
        assert np.any(full[0] != greedy[0])            # the beam does change codes on this table


@pytest.mark.parametrize("b_in", [1, 2, 5, 32])
def test_beam_step_bit_exact(be, oracle, b_in):
    n, d = 33, 64
    rng = np.random.default_rng(b_in)
    book = rng.standard_normal((256, d)).astype(np.float32)
    r = (book[rng.integers(0, 256, (n, b_in))] + np.float32(0.4) * rng.standard_normal((n, b_in, d))).astype(np.float32)
    r[:, 1:] = r[:, :1] + np.float32(0.05) * r[:, 1:]  # beams of a row near one another: their candidates interleave
    for b_out in (1, 5, 32):
        ref = rq_beam_step_ref(oracle, r, b_in, book, b_out)
        _check_step(be.rq_beam_step(r, b_in, book, b_out), ref, (b_in, b_out))
        if b_in > 1 and b_out > 1:
            assert len(np.unique(ref[1])) > 1          # more than one parent survives


@pytest.mark.parametrize("d", [8, 64])
def test_beam_path_ties_duplicates_and_midpoints(be, oracle, d):
    """Equal stage-1 distances behind the paths (a, b) and (b, a): parent slot 0 wins.  Duplicated words at j, j + 4 and
    j + 128 (the lower word wins inside a list), rows on a word, exact midpoints of two words."""
    x, cb, wa, wb, s = path_tie_case(n=64, d=d)
    book = cb[0]
    for j in (0, 1, 3, 40, 99):
        book[j + 4] = book[j]
        book[j + 128] = book[j]
    cb = np.stack([book, book])
    rng = np.random.default_rng(d)
    a, b = rng.integers(0, 256, 40), rng.integers(0, 256, 40)
    x = np.concatenate([x, book[[0, 4, 128, 1, 5, 129, 40, 44, 168]], book[a] * np.float32(0.5) + book[b] * np.float32(0.5)])
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    r1 = rq_beam_step_ref(oracle, x.reshape(n, 1, d), 1, book, 3)
    got1 = be.rq_beam_step(x, 1, book, 3)
    _check_step(got1, r1, "stage 0")
    r2 = rq_beam_step_ref(oracle, r1[0], 3, book, 3)
    _check_step(be.rq_beam_step(got1[0], 3, book, 3), r2, "stage 1")
    # the construction does what it says
    assert np.array_equal(bits(r2[3][:64, 0]), bits(r2[3][:64, 1])) and np.all(r2[1][:64, 0] == 0) and np.all(r2[1][:64, 1] == 1)
    assert list(r1[2][64]) == [0, 4, 128] and list(r1[2][65]) == [0, 4, 128] and np.all(r1[3][64:73] == 0)
    for B in (2, 3, 5):
        _check(be.rq_beam_encode(x, cb, B, want_dist=True, want_residual=True), rq_beam_encode_ref(oracle, x, cb, B), B)


@pytest.mark.parametrize("n", [300, 12])
@pytest.mark.parametrize("d", [64, 50])
def test_beam_non_finite_and_partial_fill(be, oracle, n, d):
    """d = 64: the 16-byte select kernel behind the fused sweep; d = 50: the scalar one behind the scalar lists."""
    from audio_tokens_amd.ops import ResidualQuantizer
    B, M = 5, 2
    x, book, row = partial_fill_case(n, d)
    rng = np.random.default_rng(n + d)
    cb = np.stack([book, np.float32(0.5) * rng.standard_normal((256, d)).astype(np.float32)])
    clean_x = x.copy()
    clean_x[row] = x[0]
    clean = rq_beam_encode_ref(oracle, clean_x, cb, B)
    assert not clean[3]
    x[1, 7] = np.nan
    x[2, d - 1] = np.inf
    x[3, 0] = -np.inf
    step_ref = rq_beam_step_ref(oracle, x.reshape(n, 1, d), 1, book, B)
    assert step_ref[4] and list(step_ref[2][row]) == [17, 99, 0, 0, 0] and np.all(np.isposinf(step_ref[3][1:4]))
    _check_step(be.rq_beam_step(x, 1, book, B), step_ref, "step")
    ref = rq_beam_encode_ref(oracle, x, cb, B)
    assert ref[3] and np.all(ref[0][1:4] == 0) and np.all(np.isposinf(ref[1][1:4])) and ref[0][row, 0] == 17
    got = be.rq_beam_encode(x, cb, B, want_dist=True, want_residual=True)
    _check(got, ref, "encode")
    keep = np.ones(n, bool)
    keep[1:5] = False
    assert np.array_equal(_np(got[0])[keep], clean[0][keep])       # the neighbouring rows are untouched
    assert np.array_equal(bits(_np(got[2])[keep]), bits(clean[2][keep]))
    rq = ResidualQuantizer(d, M, max_beam_size=B, backend=be)
    rq.set_centroids(cb)
    with pytest.raises(RuntimeError, match="input contains NaN's or Inf's"):
        rq.compute_codes(x)
    assert np.array_equal(rq.compute_codes(x, check_finite=False), ref[0])
    assert np.array_equal(rq.compute_codes(clean_x), clean[0])


@pytest.mark.parametrize("ksub", [1, 3, 7, 255])
def test_beam_small_codebooks(be, oracle, ksub):
    """ksub = 3, B = 5: widths 1, 3, 5; ksub = 1: one beam for ever."""
    for d, M in ((64, 3), (12, 3)):
        x, cb = _data(ksub, 150, d, M, ksub)
        assert beam_widths(5, ksub, M)[-1] == min(5, ksub ** M)
        _check(be.rq_beam_encode(x, cb, 5, want_dist=True, want_residual=True), rq_beam_encode_ref(oracle, x, cb, 5), (ksub, d))
        _check(be.rq_beam_encode(x[:7], cb, 5, want_dist=True, want_residual=True), rq_beam_encode_ref(oracle, x[:7], cb, 5),
               (ksub, d, 7))


def test_beam_rows_offset_by_one_float(be, oracle):
    x, cb = _data(3, 500, 64, 3)
    buf = torch.zeros(500 * 64 + 4, device=be.device)
    view = buf[1:1 + 500 * 64].view(500, 64)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    cbd = be._f32(cb)
    got = be.rq_beam_encode(view, cbd, 4, want_dist=True, want_residual=True)
    _check(got, rq_beam_encode_ref(oracle, x, cb, 4), "offset by one float")
    rbuf = torch.zeros(500 * 2 * 64 + 4, device=be.device)
    r = rbuf[1:1 + 500 * 2 * 64].view(500, 2, 64)
    r.copy_(torch.from_numpy(np.stack([x, x[::-1]], 1)))
    _check_step(be.rq_beam_step(r, 2, cbd[0], 4), rq_beam_step_ref(oracle, _np(r), 2, cb[0], 4), "step, offset")


def test_beam_argument_errors_and_empty_call(be):
    AT_E_INVALID = -1
    vp = ctypes.c_void_p
    x, cb = be.zeros((32, 64)), be.zeros((2, 256, 64))
    codes, r_out = be.empty((32, 2), torch.uint8), be.empty((32, 4, 64))
    parent, code, dist = be.empty((32, 4), torch.int32), be.empty((32, 4), torch.uint8), be.empty((32, 4))
    h = be.ctx.handle
    enc, step = be.lib.at_rq_beam_encode_f32, be.lib.at_rq_beam_step_f32
    px, pc, pk = vp(x.data_ptr()), vp(cb.data_ptr()), vp(codes.data_ptr())
    po, pp, pq, pd = vp(r_out.data_ptr()), vp(parent.data_ptr()), vp(code.data_ptr()), vp(dist.data_ptr())
    assert enc(h, px, 32, 64, 2, 256, pc, 4, pk, None, None, None, None) == 0
    assert step(h, px, 32, 1, 64, pc, 256, 4, po, pp, pq, pd, None, None) == 0
    torch.cuda.synchronize(be.device)
    assert enc(h, None, 0, 64, 2, 256, None, 4, None, None, None, None, None) == 0     # n == 0: no pointer is touched
    assert step(h, None, 0, 1, 64, None, 256, 4, None, None, None, None, None, None) == 0
    for a in [(None, px, 32, 64, 2, 256, pc, 4, pk), (h, px, 32, 64, 2, 256, pc, 0, pk), (h, px, 32, 64, 2, 256, pc, 33, pk),
              (h, px, 32, 64, 2, 0, pc, 4, pk), (h, px, 32, 64, 2, 257, pc, 4, pk), (h, px, -1, 64, 2, 256, pc, 4, pk),
              (h, px, 32, 0, 2, 256, pc, 4, pk), (h, px, 32, 64, 0, 256, pc, 4, pk), (h, None, 32, 64, 2, 256, pc, 4, pk),
              (h, px, 32, 64, 2, 256, None, 4, pk), (h, px, 32, 64, 2, 256, pc, 4, None)]:
        assert enc(*a, None, None, None, None) == AT_E_INVALID, a
        assert b"at_rq_beam_encode_f32" in be.lib.at_last_error()
    assert enc(h, px, 32, 64, 2, 256, pc, 4, pk, None, vp(x.data_ptr() + 64), None, None) == AT_E_INVALID   # overlaps x
    assert b"overlaps" in be.lib.at_last_error()
    for a in [(None, px, 32, 1, 64, pc, 256, 4, po, pp, pq, pd), (h, px, 32, 0, 64, pc, 256, 4, po, pp, pq, pd),
              (h, px, 32, 33, 64, pc, 256, 4, po, pp, pq, pd), (h, px, 32, 1, 64, pc, 256, 0, po, pp, pq, pd),
              (h, px, 32, 1, 64, pc, 256, 33, po, pp, pq, pd), (h, px, 32, 1, 64, pc, 3, 4, po, pp, pq, pd),   # b_out > b_in * ksub
              (h, px, 32, 1, 0, pc, 256, 4, po, pp, pq, pd), (h, px, 32, 1, 64, pc, 257, 4, po, pp, pq, pd),
              (h, px, -1, 1, 64, pc, 256, 4, po, pp, pq, pd), (h, None, 32, 1, 64, pc, 256, 4, po, pp, pq, pd),
              (h, px, 32, 1, 64, None, 256, 4, po, pp, pq, pd), (h, px, 32, 1, 64, pc, 256, 4, None, pp, pq, pd),
              (h, px, 32, 1, 64, pc, 256, 4, po, None, pq, pd), (h, px, 32, 1, 64, pc, 256, 4, po, pp, None, pd),
              (h, px, 32, 1, 64, pc, 256, 4, po, pp, pq, None)]:
        assert step(*a, None, None) == AT_E_INVALID, a
        assert b"at_rq_beam_step_f32" in be.lib.at_last_error()
    assert step(h, px, 32, 1, 64, pc, 256, 4, vp(x.data_ptr() + 64), pp, pq, pd, None, None) == AT_E_INVALID
    assert b"overlaps" in be.lib.at_last_error()
    with pytest.raises(ValueError):
        be.rq_beam_encode(x, be.zeros((2, 256, 32)), 4)
    got = be.rq_beam_encode(be.zeros((0, 64)), cb, 4, want_dist=True, want_residual=True)
    assert tuple(got[0].shape) == (0, 2) and tuple(got[1].shape) == (0, 2) and tuple(got[2].shape) == (0, 64)
    assert int(got[3].item()) == 0


def test_beam_without_distances_or_residual_and_two_streams_at_once(be, oracle):
    x1, c1 = _data(11, 6000, 64, 3)
    x2, c2 = _data(12, 2500, 128, 2)
    t = [be._f32(a) for a in (x1, c1, x2, c2)]
    want = [be.rq_beam_encode(t[0], t[1], 5, want_dist=True, want_residual=True),
            be.rq_beam_encode(t[2], t[3], 3, want_dist=True, want_residual=True)]
    _check((want[0][0][:400], want[0][1][:400], want[0][2][:400], want[0][3]), rq_beam_encode_ref(oracle, x1[:400], c1, 5), "1")
    _check((want[1][0][:400], want[1][1][:400], want[1][2][:400], want[1][3]), rq_beam_encode_ref(oracle, x2[:400], c2, 3), "2")
    codes, dist, res, bad = be.rq_beam_encode(t[0], t[1], 5)
    assert dist is None and res is None and torch.equal(codes, want[0][0]) and int(bad.item()) == 0
    codes, dist, res, bad = be.rq_beam_encode(t[2], t[3], 3, want_dist=True)
    assert res is None and torch.equal(codes, want[1][0]) and torch.equal(dist.view(torch.int32), want[1][1].view(torch.int32))
    torch.cuda.synchronize(be.device)
    s1, s2 = torch.cuda.Stream(be.device), torch.cuda.Stream(be.device)
    s1.wait_stream(torch.cuda.current_stream(be.device))
    s2.wait_stream(torch.cuda.current_stream(be.device))
    with torch.cuda.stream(s1):
        r1 = be.rq_beam_encode(t[0], t[1], 5, want_dist=True, want_residual=True)
        r3 = be.rq_beam_encode(t[0], t[1], 5, want_dist=True, want_residual=True)
    with torch.cuda.stream(s2):
        r2 = be.rq_beam_encode(t[2], t[3], 3, want_dist=True, want_residual=True)
        r4 = be.rq_beam_encode(t[2], t[3], 3, want_dist=True, want_residual=True)
    torch.cuda.synchronize(be.device)
    for got, ref in zip((r1, r2, r3, r4), (want[0], want[1], want[0], want[1])):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))
        assert torch.equal(got[2].view(torch.int32), ref[2].view(torch.int32))


def test_beam_encode_across_row_blocks(be):
    """B = 32, d = 128, M = 2: a row of a block takes 2 * 4 * 32 * 128 (two residual buffers) + 12 * 32 * 32 (lists) +
    9 * 2 * 32 (records) = 45 632 bytes of workspace, so the 256 MiB budget holds 5882 rows.  n = 2 * 5882 + 7 would
    leave a block of 7 rows, fewer than the 20 below which the search takes its other distance form: the block in front
    of it gives 20 rows up.  The same rows encoded in two halves by the caller (5886 = 5882 + 4 rows: the same rule) give
    the same bits, and so does the stage-by-stage composition from rq_beam_step, which has no blocks."""
    n, d, M, B = 2 * 5882 + 7, 128, 2, 32
    g = torch.Generator(device=be.device).manual_seed(5)
    cb = torch.randn(M, 256, d, device=be.device, generator=g)
    cb[1] *= 0.5
    x = (cb[0][torch.randint(0, 256, (n,), device=be.device, generator=g)] +
         cb[1][torch.randint(0, 256, (n,), device=be.device, generator=g)] +
         0.2 * torch.randn(n, d, device=be.device, generator=g)).contiguous()
    x[::2] = torch.randn((n + 1) // 2, d, device=be.device, generator=g)   # rows near no sum of words: the beams matter
    whole = be.rq_beam_encode(x, cb, B, want_dist=True, want_residual=True)
    h = 5886
    parts = [be.rq_beam_encode(x[:h], cb, B, want_dist=True, want_residual=True),
             be.rq_beam_encode(x[h:], cb, B, want_dist=True, want_residual=True)]
    assert int(whole[3].item()) == 0
    for j in range(3):
        both = torch.cat([parts[0][j], parts[1][j]], 0)
        assert torch.equal(whole[j].view(torch.uint8), both.view(torch.uint8)), j
    r1, _, c1, d1, _ = be.rq_beam_step(x, 1, cb[0], B)
    r2, p2, c2, d2, _ = be.rq_beam_step(r1, B, cb[1], B)
    first = p2[:, 0].to(torch.int64).unsqueeze(1)
    assert torch.equal(whole[0][:, 1], c2[:, 0]) and torch.equal(whole[0][:, 0], c1.gather(1, first)[:, 0])
    assert torch.equal(whole[1][:, 1].contiguous().view(torch.int32), d2[:, 0].contiguous().view(torch.int32))
    assert torch.equal(whole[2].view(torch.int32), r2[:, 0].contiguous().view(torch.int32))
    assert len(torch.unique(p2[:, 0])) > 1                 # slot 0 does come from other parents than the greedy one


def test_residual_quantizer_beam_call_forms_and_training(be, oracle):
    from audio_tokens_amd.ops import Kmeans, ResidualQuantizer
    x, cb = _data(9, 400, 64, 3)
    cr, dr, rr, _ = rq_beam_encode_ref(oracle, x, cb, 5)
    rq = ResidualQuantizer(64, 3, max_beam_size=5, backend=be)
    rq.set_centroids(cb)
    codes, dist, res = rq.compute_codes(x, return_distances=True, return_residual=True)   # host in, numpy out
    assert isinstance(codes, np.ndarray) and codes.dtype == np.uint8
    assert np.array_equal(codes, cr) and np.array_equal(bits(dist), bits(dr)) and np.array_equal(bits(res), bits(rr))
    xd = torch.from_numpy(x).to(be.device)
    codes_d = rq.compute_codes(xd)
    assert codes_d.device == xd.device and np.array_equal(_np(codes_d), cr)
    by_stages = rq._encode_by_stages(xd, rq.centroids_device, True, True)            # rq_beam_step per stage, torch walk
    _check(by_stages, (cr, dr, rr, False), "by stages")
    empty = rq.compute_codes(np.zeros((0, 64), np.float32), return_distances=True, return_residual=True)
    assert [a.shape for a in empty] == [(0, 3), (0, 3), (0, 64)]
    with pytest.raises(NotImplementedError):
        ResidualQuantizer(64, 3, max_beam_size=33, backend=be)

    rng = np.random.default_rng(8)
    xt = rng.standard_normal((6000, 64)).astype(np.float32)
    tr = ResidualQuantizer(64, 3, niter=3, max_beam_size=3, backend=be)
    tr.train(xt)
    r, b = be._f32(xt), 1
    for m in range(3):
        km = Kmeans(64, 256, niter=3, seed=1234, backend=be)
        km.train(r.reshape(-1, 64))
        assert np.array_equal(bits(tr.centroids[m]), bits(km.centroids)), m
        if m < 2:
            r = be.rq_beam_step(r, b, km.centroids_device, 3)[0]
            b = 3
    assert tuple(r.shape) == (6000, 3, 64)
