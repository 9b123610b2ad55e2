"""ops.ResidualQuantizer / at_rq_encode_f32 / at_rq_decode_f32 on the MI355X, bit for bit against tests/rq_ref.py (one
oracle search per stage on the running residual) and against the existing kernels (be.assign per stage plus a torch
subtraction, Kmeans per stage)."""
import ctypes

import numpy as np
import pytest
import torch

from rq_ref import rq_decode_ref, rq_encode_ref

pytestmark = pytest.mark.gpu

# (d, M): fused at d = 64 (one chunk) and 128 (two); general (one at_assign_f32 per stage) everywhere else: d = 8, 12,
# 32 (any-d sweep), 50 (scalar sweep: d % 4 != 0), 640 (ten chunks); M = 5: more than four stages, codes stored as bytes
SHAPES = [(64, 1), (64, 2), (64, 5), (64, 8), (128, 4), (8, 3), (12, 2), (50, 2), (32, 4), (640, 2)]
NS = [1, 19, 20, 31, 32, 33, 127, 128, 129, 4097]
OFFS = (4, 16, 32, 128)   # register, accumulator, half-wave / 32-centroid and 128-centroid (tile) boundaries


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _check(got, ref, label=""):
    """got: (codes, dist, residual, bad) of be.rq_encode; ref: rq_encode_ref's."""
    codes, dist, res, bad = _np(got[0]), _np(got[1]), _np(got[2]), int(got[3].item())
    cr, dr, rr, br = ref
    assert codes.dtype == np.uint8 and codes.shape == cr.shape and dist.shape == dr.shape and res.shape == rr.shape, label
    wrong = np.argwhere((codes != cr) | (bits(dist) != bits(dr)))
    assert wrong.size == 0, (label, wrong[:5], codes[tuple(wrong[0])], cr[tuple(wrong[0])], dist[tuple(wrong[0])],
                             dr[tuple(wrong[0])])
    wrong = np.argwhere(bits(res) != bits(rr))
    assert wrong.size == 0, (label, "residual", wrong[:5], res[tuple(wrong[0])], rr[tuple(wrong[0])])
    assert bad == int(br), label


def _data(seed, n, d, M, ksub=256):
    """Codebooks that get finer stage by stage, and rows near sums of one word per stage."""
    rng = np.random.default_rng(seed)
    cb = rng.standard_normal((M, ksub, d)).astype(np.float32)
    for m in range(M):
        cb[m] *= np.float32(0.5 ** m)
    x = rng.standard_normal((n, d)).astype(np.float32)
    if n > 3:                                      # three quarters of the rows close to a sum of words
        q = 3 * n // 4
        pick = rng.integers(0, ksub, (q, M))
        near = np.zeros((q, d), np.float32)
        for m in range(M):
            near = near + cb[m][pick[:, m]]
        x[:q] = (near + np.float32(0.5 ** M * 0.3) * x[:q]).astype(np.float32)
    return x, cb


@pytest.mark.parametrize("d,M", SHAPES)
def test_rq_grid_bit_exact(be, oracle, d, M):
    xall, cb = _data(d * 31 + M, max(NS), d, M)
    cbd = be._f32(cb)
    full = rq_encode_ref(oracle, xall, cb)         # rows are independent: a call of n >= 20 rows is a prefix of it
    for n in NS:
        x = xall[:n]
        ref = rq_encode_ref(oracle, x, cb) if n < 20 else (full[0][:n], full[1][:n], full[2][:n], full[3])
        _check(be.rq_encode(x, cbd, want_dist=True, want_residual=True), ref, (d, M, n))
    if d == 64 and M == 8:
        assert len(np.unique(full[0][:, 7])) > 100         # the late stages still choose among their words


def _grid_books(rng, d, M):
    """Words on a dyadic grid, stage m in steps of 2^-(3 m): sums of one word per stage, and the residuals behind them,
    are exact in fp32, and equal distances abound.  Duplicated words across every boundary of the layout."""
    cb = np.empty((M, 256, d), np.float32)
    for m in range(M):
        cb[m] = rng.integers(-4, 5, (256, d)).astype(np.float32) * np.float32(0.125 ** m)
        for j in (0, 1, 3, 5, 17, 40, 70, 99, 125):
            for off in OFFS:
                if j + off < 256:
                    cb[m, j + off] = cb[m, j]
    return cb


@pytest.mark.parametrize("d,M", [(64, 4), (128, 2), (8, 3)])
def test_rq_ties_and_near_ties(be, oracle, d, M):
    """Duplicated words at j, j+4, j+16, j+32, j+128 in every stage (the lowest index wins), rows equal to a stage-0 word
    (zero residual into stage 1), rows equal to word_0 + word_1 (zero residual into stage 2), and exact midpoints of two
    words with tests/test_gpu_knn.py's perturbations."""
    rng = np.random.default_rng(d + M)
    n = 3000
    cb = _grid_books(rng, d, M)
    first = np.array([[min(i for i in range(256) if np.array_equal(cb[m, i], cb[m, j])) for j in range(256)]
                      for m in range(M)])
    assert (first[0] != np.arange(256)).sum() >= 30
    a, b = rng.integers(0, 256, n), rng.integers(0, 256, n)
    t = np.float32(0.5) + rng.choice([0.0, 1e-7, -1e-7, 1e-6, -1e-5, 1e-4, -1e-3], n).astype(np.float32)
    x = cb[0][a] * t[:, None] + cb[0][b] * (np.float32(1) - t)[:, None]
    x[:300] = cb[0][a[:300]] * np.float32(0.5) + cb[0][b[:300]] * np.float32(0.5)     # exact midpoints
    x[300:556] = cb[0]                                                                   # row j on word j
    x[556:812] = cb[0][::-1]
    w1 = rng.integers(0, 256, 256)
    x[812:1068] = cb[0] + cb[1][w1]                                                      # word_0 + word_1, exact
    x = np.ascontiguousarray(x, dtype=np.float32)
    ref = rq_encode_ref(oracle, x, cb)
    _check(be.rq_encode(x, cb, want_dist=True, want_residual=True), ref, (d, M))
    # the construction does what it says: a row on word j is at distance 0 and gets the first copy of j, never a later
    # duplicate, and goes into stage 1 as zero, where it takes the first of the words nearest to the origin
    assert np.all(ref[1][300:556, 0] == 0) and np.array_equal(ref[0][300:556, 0], first[0])
    assert np.any(ref[0][300:556, 0] != np.arange(256))
    norms = (cb[1].astype(np.float64) ** 2).sum(1)
    assert np.all(ref[0][300:556, 1] == int(np.argmin(norms)))
    assert np.array_equal(ref[0][812:1068, 0], first[0]) and np.all(ref[1][812:1068, 1] == 0)
    assert np.array_equal(ref[0][812:1068, 1], first[1][w1])
    if M > 2:
        norms2 = (cb[2].astype(np.float64) ** 2).sum(1)
        assert np.all(ref[0][812:1068, 2] == int(np.argmin(norms2))) and np.all(ref[1][812:1068, 2] == norms2.min())


@pytest.mark.parametrize("n", [300, 12])
@pytest.mark.parametrize("d", [64, 12])
def test_rq_non_finite_and_degenerate(be, oracle, n, d):
    M = 3
    x, cb = _data(77, n, d, M)
    clean = rq_encode_ref(oracle, x, cb)
    assert not clean[3]
    cb[:, 9] = 0.0                                 # zero words, zero rows
    cb[1, 200] = -3e19                             # |c|^2 overflows: never the nearest, the others still are
    x[0] = 0.0
    ref0 = rq_encode_ref(oracle, x, cb)
    assert not ref0[3] and np.all(ref0[0][0] == 9) and np.all(ref0[1][0] == 0) and np.all(ref0[2][0] == 0)
    assert not np.any(ref0[0][:, 1] == 200)
    _check(be.rq_encode(x, cb, want_dist=True, want_residual=True), ref0, "degenerate")
    x[2, 7] = np.nan
    x[3, d - 1] = np.inf
    x[4, 0] = -np.inf
    x[5] = 3e19                                    # |x|^2 overflows
    x[6, 2:10] = 1e19                              # large, finite: |x|^2 = 8e38 overflows as well
    x[7, 2:10] = 1e18                              # large and still finite
    ref = rq_encode_ref(oracle, x, cb)
    assert ref[3] and np.all(ref[0][2:7] == 0) and np.all(np.isposinf(ref[1][2:7]))     # flagged at every stage
    assert np.all(np.isfinite(ref[1][7])) and np.isnan(ref[2][2, 7]) and np.isposinf(ref[2][3, d - 1])
    got = be.rq_encode(x, cb, want_dist=True, want_residual=True)
    _check(got, ref, "non-finite")
    keep = np.ones(n, bool)
    keep[2:8] = False
    assert np.array_equal(_np(got[0])[keep], ref0[0][keep])       # the neighbouring rows are untouched
    assert np.array_equal(bits(_np(got[2])[keep]), bits(ref0[2][keep]))


@pytest.mark.parametrize("ksub", [1, 7, 129, 255])   # 129: a second tile with one real word
def test_rq_small_codebooks(be, oracle, ksub):
    for d, M in ((64, 3), (128, 2), (12, 3)):
        x, cb = _data(ksub, 300, d, M, ksub)
        _check(be.rq_encode(x, cb, want_dist=True, want_residual=True), rq_encode_ref(oracle, x, cb), (ksub, d, M))
        _check(be.rq_encode(x[:7], cb, want_dist=True, want_residual=True), rq_encode_ref(oracle, x[:7], cb),
               (ksub, d, M, 7))
        codes = rq_encode_ref(oracle, x, cb)[0]
        assert np.array_equal(bits(_np(be.rq_decode(codes, cb))), bits(rq_decode_ref(codes, cb)))


def test_rq_unaligned_rows_take_the_general_path(be, oracle):
    x, cb = _data(3, 1000, 64, 4)
    buf = torch.zeros(1000 * 64 + 4, device=be.device)
    view = buf[1:1 + 1000 * 64].view(1000, 64)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    cbd = be._f32(cb)
    got = be.rq_encode(view, cbd, want_dist=True, want_residual=True)
    _check(got, rq_encode_ref(oracle, x, cb), "offset by one float")
    aligned = be.rq_encode(x, cbd, want_dist=True, want_residual=True)
    assert torch.equal(got[0], aligned[0]) and torch.equal(got[1].view(torch.int32), aligned[1].view(torch.int32))
    assert torch.equal(got[2].view(torch.int32), aligned[2].view(torch.int32))


def test_rq_argument_errors_empty_call_and_bad_codes(be):
    AT_E_INVALID = -1
    vp = ctypes.c_void_p
    x, cb = be.zeros((32, 64)), be.zeros((4, 256, 64))
    codes, out = be.empty((32, 4), torch.uint8), be.empty((32, 64))
    h = be.ctx.handle
    enc, dec = be.lib.at_rq_encode_f32, be.lib.at_rq_decode_f32
    px, pc, pk, po = vp(x.data_ptr()), vp(cb.data_ptr()), vp(codes.data_ptr()), vp(out.data_ptr())
    assert enc(h, px, 32, 64, 4, 256, pc, pk, None, None, None, None) == 0
    assert dec(h, pk, 32, 64, 4, 256, pc, po, None) == 0
    torch.cuda.synchronize(be.device)
    assert enc(h, None, 0, 64, 4, 256, None, None, None, None, None, None) == 0     # n == 0: no pointer is touched
    assert dec(h, None, 0, 64, 4, 256, None, None, None) == 0
    cases = [(None, px, 32, 64, 4, 256, pc, pk), (h, px, 32, 64, 4, 0, pc, pk), (h, px, 32, 64, 4, 257, pc, pk),
             (h, px, -1, 64, 4, 256, pc, pk), (h, px, 32, 0, 4, 256, pc, pk), (h, px, 32, 64, 0, 256, pc, pk),
             (h, None, 32, 64, 4, 256, pc, pk), (h, px, 32, 64, 4, 256, None, pk), (h, px, 32, 64, 4, 256, pc, None)]
    for a in cases:
        assert enc(*a, None, None, None, None) == AT_E_INVALID, a
        assert b"at_rq_encode_f32" in be.lib.at_last_error()
    assert enc(h, px, 32, 64, 4, 256, pc, pk, None, vp(x.data_ptr() + 64), None, None) == AT_E_INVALID   # overlaps x
    assert b"overlaps" in be.lib.at_last_error()
    for a in [(None, pk, 32, 64, 4, 256, pc, po), (h, pk, 32, 64, 0, 256, pc, po), (h, pk, 32, 64, 4, 300, pc, po),
              (h, pk, 32, 0, 4, 256, pc, po), (h, None, 32, 64, 4, 256, pc, po), (h, pk, 32, 64, 4, 256, None, po),
              (h, pk, 32, 64, 4, 256, pc, None)]:
        assert dec(*a, None) == AT_E_INVALID, a
        assert b"at_rq_decode_f32" in be.lib.at_last_error()
    with pytest.raises(ValueError):
        be.rq_encode(x, be.zeros((4, 256, 32)))
    got = be.rq_encode(be.zeros((0, 64)), cb, want_dist=True, want_residual=True)
    assert tuple(got[0].shape) == (0, 4) and tuple(got[1].shape) == (0, 4) and tuple(got[2].shape) == (0, 64)
    assert int(got[3].item()) == 0
    # a code >= ksub makes that row NaN rather than reading past the table; the 16-byte and the scalar decoder
    rng = np.random.default_rng(2)
    for d in (64, 10):
        cb7 = rng.standard_normal((3, 7, d)).astype(np.float32)
        c = rng.integers(0, 7, (50, 3)).astype(np.uint8)
        c[4, 0], c[9, 2], c[20, 1] = 7, 255, 100
        dec_out = _np(be.rq_decode(c, cb7))
        hit = np.zeros(50, bool)
        hit[[4, 9, 20]] = True
        assert np.all(np.isnan(dec_out[hit]))
        c[hit] = 0
        assert np.array_equal(bits(dec_out[~hit]), bits(rq_decode_ref(c, cb7)[~hit]))


def test_rq_without_distances_or_residual_and_two_streams_at_once(be, oracle):
    x1, c1 = _data(11, 20000, 64, 4)
    x2, c2 = _data(12, 5000, 128, 3)
    t = [be._f32(a) for a in (x1, c1, x2, c2)]
    want = [be.rq_encode(t[0], t[1], want_dist=True, want_residual=True),
            be.rq_encode(t[2], t[3], want_dist=True, want_residual=True)]
    _check(want[0], rq_encode_ref(oracle, x1, c1), "stream 1 shape")
    _check(want[1], rq_encode_ref(oracle, x2, c2), "stream 2 shape")
    codes, dist, res, bad = be.rq_encode(t[0], t[1])
    assert dist is None and res is None and torch.equal(codes, want[0][0]) and int(bad.item()) == 0
    codes, dist, res, bad = be.rq_encode(t[2], t[3], want_dist=True)
    assert res is None and torch.equal(codes, want[1][0]) and torch.equal(dist.view(torch.int32), want[1][1].view(torch.int32))
    codes, dist, res, bad = be.rq_encode(t[0][:, :50].contiguous(), t[1][:, :, :50].contiguous())   # general path
    assert dist is None and res is None
    assert np.array_equal(_np(codes), rq_encode_ref(oracle, x1[:, :50], c1[:, :, :50])[0])
    torch.cuda.synchronize(be.device)
    s1, s2 = torch.cuda.Stream(be.device), torch.cuda.Stream(be.device)
    s1.wait_stream(torch.cuda.current_stream(be.device))
    s2.wait_stream(torch.cuda.current_stream(be.device))
    with torch.cuda.stream(s1):
        r1 = be.rq_encode(t[0], t[1], want_dist=True, want_residual=True)
        r3 = be.rq_encode(t[0], t[1], want_dist=True, want_residual=True)
    with torch.cuda.stream(s2):
        r2 = be.rq_encode(t[2], t[3], want_dist=True, want_residual=True)
        r4 = be.rq_encode(t[2], t[3], want_dist=True, want_residual=True)
    torch.cuda.synchronize(be.device)
    for got, ref in zip((r1, r2, r3, r4), (want[0], want[1], want[0], want[1])):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))
        assert torch.equal(got[2].view(torch.int32), ref[2].view(torch.int32))


def test_residual_quantizer_call_forms(be, oracle):
    from audio_tokens_amd.ops import ResidualQuantizer
    x, cb = _data(9, 3000, 64, 4)
    cr, dr, rr, _ = rq_encode_ref(oracle, x, cb)
    rq = ResidualQuantizer(64, 4, backend=be)
    with pytest.raises(RuntimeError, match="not trained"):
        rq.compute_codes(x)
    rq.set_centroids(cb)
    codes, dist, res = rq.compute_codes(x, return_distances=True, return_residual=True)   # host in, numpy out
    assert isinstance(codes, np.ndarray) and codes.dtype == np.uint8 and dist.dtype == np.float32 and res.dtype == np.float32
    assert np.array_equal(codes, cr) and np.array_equal(bits(dist), bits(dr)) and np.array_equal(bits(res), bits(rr))
    xd = torch.from_numpy(x).to(be.device)
    codes_d = rq.compute_codes(xd)                                            # device in, device out
    assert codes_d.device == xd.device and codes_d.dtype == torch.uint8 and np.array_equal(_np(codes_d), cr)
    codes_d2, res_d = rq.compute_codes(xd, return_residual=True)
    assert res_d.device == xd.device and np.array_equal(bits(_np(res_d)), bits(rr)) and torch.equal(codes_d2, codes_d)
    assert np.array_equal(rq.compute_codes(x.astype(np.float64)), cr)         # float64: converted to float32 first
    wide = torch.zeros((3000, 128), device=be.device)
    wide[:, ::2] = xd
    assert np.array_equal(_np(rq.compute_codes(wide[:, ::2])), cr)            # strided device view
    empty = rq.compute_codes(np.zeros((0, 64), np.float32), return_distances=True, return_residual=True)
    assert [a.shape for a in empty] == [(0, 4), (0, 4), (0, 64)]
    out = rq.decode(codes)                                                    # decode: host and device
    assert isinstance(out, np.ndarray) and np.array_equal(bits(out), bits(rq_decode_ref(cr, cb)))
    out_d = rq.decode(codes_d)
    assert out_d.device == xd.device and np.array_equal(bits(_np(out_d)), bits(out))
    bad = x.copy()
    bad[5, 9] = np.nan
    with pytest.raises(RuntimeError, match="input contains NaN's or Inf's"):
        rq.compute_codes(bad)
    got = rq.compute_codes(bad, check_finite=False)
    assert np.all(got[5] == 0) and np.array_equal(np.delete(got, 5, 0), np.delete(cr, 5, 0))
    rq10 = ResidualQuantizer(10, 3, backend=be)                               # general encoder, scalar decoder
    x10, cb10 = _data(10, 500, 10, 3)
    rq10.set_centroids(cb10)
    c10 = rq10.compute_codes(x10)
    assert np.array_equal(c10, rq_encode_ref(oracle, x10, cb10)[0])
    assert np.array_equal(bits(rq10.decode(c10)), bits(rq_decode_ref(c10, cb10)))


@pytest.mark.parametrize("d,M", [(64, 8), (128, 4)])
def test_rq_large_against_the_assign_composition(be, d, M):
    """n = 2^18: the fused call against one be.assign per stage plus a torch subtraction, on the device."""
    n = 1 << 18
    g = torch.Generator(device=be.device).manual_seed(4)
    cb = torch.randn(M, 256, d, device=be.device, generator=g)
    x = torch.zeros(n, d, device=be.device)
    for m in range(M):
        cb[m] *= 0.5 ** m
        x += cb[m][torch.randint(0, 256, (n,), device=be.device, generator=g)]
    x = (x + 0.5 ** M * 0.3 * torch.randn(n, d, device=be.device, generator=g)).contiguous()
    codes, dist, res, bad = be.rq_encode(x, cb, want_dist=True, want_residual=True)
    assert int(bad.item()) == 0
    r = x
    for m in range(M):
        ids, dis = be.assign(r, cb[m])
        assert torch.equal(codes[:, m].to(torch.int64), ids), m
        assert torch.equal(dist[:, m].contiguous().view(torch.int32), dis.view(torch.int32)), m
        r = r - cb[m][ids]
    assert torch.equal(res.view(torch.int32), r.view(torch.int32))
    out = be.rq_decode(codes, cb)
    want = cb[0][codes[:, 0].to(torch.int64)].clone()
    for m in range(1, M):
        want = want + cb[m][codes[:, m].to(torch.int64)]
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    assert len(torch.unique(codes[:, M - 1])) > 200


def test_residual_quantizer_train_on_the_device(be):
    from audio_tokens_amd.ops import Kmeans, ResidualQuantizer
    rng = np.random.default_rng(8)
    x = rng.standard_normal((20000, 64)).astype(np.float32)
    rq = ResidualQuantizer(64, 3, niter=4, backend=be)
    rq.train(x)
    assert rq.is_trained and rq.centroids.shape == (3, 256, 64)
    r = be._f32(x)
    for m in range(3):
        km = Kmeans(64, 256, niter=4, seed=1234, backend=be)
        km.train(r)
        assert np.array_equal(bits(rq.centroids[m]), bits(km.centroids)), m
        ids, _ = be.assign(r, km.centroids_device)
        r = r - km.centroids_device[ids]
    codes, dist = rq.compute_codes(x, return_distances=True)
    assert codes.shape == (20000, 3) and len(np.unique(codes)) > 200
    assert dist[:, 2].sum() < dist[:, 1].sum() < dist[:, 0].sum()
