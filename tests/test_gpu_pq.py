"""ops.ProductQuantizer / at_pq_encode_f32 / at_pq_decode_f32 on the MI355X, bit for bit against tests/pq_ref.py (one
oracle search per sub-space) and against the existing kernels (be.assign on contiguous slices, Kmeans per sub-space)."""
import ctypes

import numpy as np
import pytest
import torch

from pq_ref import pq_decode_ref, pq_encode_ref

pytestmark = pytest.mark.gpu

# (d, M): fused with the sub-vector in registers (dsub 4, 8, 16), fused with a run-time dsub (8/1: one sub-space;
# 24/2: dsub = 12), general (12/4: dsub = 3; 640/8: the image does not fit the LDS)
SHAPES = [(8, 1), (8, 2), (16, 2), (32, 8), (64, 8), (64, 4), (64, 16), (128, 8), (128, 32), (24, 2), (12, 4), (640, 8)]
NS = [1, 19, 20, 31, 32, 33, 127, 128, 129, 4097]
OFFS = (4, 16, 32, 128)   # register, accumulator, half-wave / 32-centroid and 128-centroid (pass) boundaries


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _check(got, ref, label=""):
    """got: (codes, dist, bad) of be.pq_encode; ref: pq_encode_ref's."""
    codes, dist, bad = _np(got[0]), _np(got[1]), int(got[2].item())
    cr, dr, br = ref
    assert codes.dtype == np.uint8 and codes.shape == cr.shape and dist.shape == dr.shape, label
    wrong = np.argwhere((codes != cr) | (bits(dist) != bits(dr)))
    assert wrong.size == 0, (label, wrong[:5], codes[tuple(wrong[0])], cr[tuple(wrong[0])], dist[tuple(wrong[0])],
                             dr[tuple(wrong[0])])
    assert bad == int(br), label


def _data(seed, n, d, M, ksub=256):
    rng = np.random.default_rng(seed)
    dsub = d // M
    cb = rng.standard_normal((M, ksub, dsub)).astype(np.float32)
    x = rng.standard_normal((n, d)).astype(np.float32)
    if n > 3:                                      # a quarter of the rows close to codebook rows
        q = n // 4
        pick = rng.integers(0, ksub, (q, M))
        near = np.concatenate([cb[m][pick[:, m]] for m in range(M)], 1)
        x[:q] = (near + np.float32(0.05) * x[:q]).astype(np.float32)
    return x, cb


@pytest.mark.parametrize("d,M", SHAPES)
def test_pq_grid_bit_exact(be, oracle, d, M):
    xall, cb = _data(d * 31 + M, max(NS), d, M)
    cbd = be._f32(cb)
    for n in NS:
        x = xall[:n]
        _check(be.pq_encode(x, cbd, want_dist=True), pq_encode_ref(oracle, x, cb), (d, M, n))


@pytest.mark.parametrize("d,M", [(64, 8), (32, 8), (24, 2), (64, 4), (12, 4)])
def test_pq_ties_and_near_ties(be, oracle, d, M):
    """Duplicated codebook rows across every boundary of the layout, rows equal to codebook rows (the clamp at 0 makes
    ties among the duplicates: the lowest index wins), and exact midpoints of two codebook rows with tests/test_gpu_knn.py's
    perturbations."""
    rng = np.random.default_rng(d + M)
    dsub, n = d // M, 3000
    cb = rng.standard_normal((M, 256, dsub)).astype(np.float32)
    for j in (0, 1, 3, 5, 17, 40, 70, 99, 125):
        for off in OFFS:
            if j + off < 256:
                cb[:, j + off] = cb[:, j]
    first = np.array([min(i for i in range(256) if np.array_equal(cb[0, i], cb[0, j])) for j in range(256)])
    assert (first != np.arange(256)).sum() >= 30
    a, b = rng.integers(0, 256, (n, M)), rng.integers(0, 256, (n, M))
    t = np.float32(0.5) + rng.choice([0.0, 1e-7, -1e-7, 1e-6, -1e-5, 1e-4, -1e-3], (n, M)).astype(np.float32)
    x = np.empty((n, d), np.float32)
    for m in range(M):
        sl = slice(m * dsub, (m + 1) * dsub)
        x[:, sl] = cb[m][a[:, m]] * t[:, m, None] + cb[m][b[:, m]] * (np.float32(1) - t[:, m])[:, None]
        x[:300, sl] = cb[m][a[:300, m]] * np.float32(0.5) + cb[m][b[:300, m]] * np.float32(0.5)   # exact midpoints
        x[300:556, sl] = cb[m]                                                                     # row j on word j
        x[556:812, sl] = cb[m][::-1]
    ref = pq_encode_ref(oracle, x, cb)
    _check(be.pq_encode(x, cb, want_dist=True), ref, (d, M))
    # the construction does what it says: a row on word j is at distance 0 and gets the first copy of j (or a lower
    # word that the clamp also puts at 0), never a later duplicate
    assert np.all(ref[1][300:556] == 0) and np.all(ref[0][300:556] <= first[:, None])
    assert np.any(ref[0][300:556] != np.arange(256)[:, None])


@pytest.mark.parametrize("n", [300, 12])
def test_pq_non_finite_and_degenerate(be, oracle, n):
    d, M, dsub = 64, 8, 8
    x, cb = _data(77, n, d, M)
    clean = pq_encode_ref(oracle, x, cb)
    assert not clean[2]
    cb[:, 9] = 0.0                                 # zero codebook rows, zero rows
    cb[2, 200] = 3e19                              # |c|^2 overflows: never the nearest, the others still are
    x[0] = 0.0
    x[1, 8:16] = 0.0
    ref0 = pq_encode_ref(oracle, x, cb)
    assert not ref0[2] and np.all(ref0[0][0] == 9)
    _check(be.pq_encode(x, cb, want_dist=True), ref0, "degenerate")
    x[2, 17] = np.nan                              # sub-space 2
    x[3, 63] = np.inf                              # sub-space 7
    x[4, 0] = -np.inf                              # sub-space 0
    x[5, 40:48] = 3e19                             # |x|^2 overflows in sub-space 5
    x[6, 24:32] = 1e19                             # large, finite: |x|^2 = 8e38 overflows as well
    x[7, 24:32] = 1e18                             # large and still finite
    ref = pq_encode_ref(oracle, x, cb)
    assert ref[2] and ref[0][2, 2] == 0 and np.isposinf(ref[1][2, 2]) and np.isposinf(ref[1][5, 5])
    assert np.isfinite(ref[1][7, 3])
    got = be.pq_encode(x, cb, want_dist=True)
    _check(got, ref, "non-finite")
    keep = np.ones((n, M), bool)
    keep[2, 2] = keep[3, 7] = keep[4, 0] = keep[5, 5] = keep[6, 3] = keep[7, 3] = False
    assert np.array_equal(_np(got[0])[keep], ref0[0][keep])       # the other sub-spaces of those rows are untouched


@pytest.mark.parametrize("ksub", [1, 7, 255])
def test_pq_small_codebooks(be, oracle, ksub):
    for d, M in ((64, 8), (12, 4)):
        x, cb = _data(ksub, 300, d, M, ksub)
        _check(be.pq_encode(x, cb, want_dist=True), pq_encode_ref(oracle, x, cb), (ksub, d, M))
        _check(be.pq_encode(x[:7], cb, want_dist=True), pq_encode_ref(oracle, x[:7], cb), (ksub, d, M, 7))
        codes = pq_encode_ref(oracle, x, cb)[0]
        assert np.array_equal(bits(_np(be.pq_decode(codes, cb))), bits(pq_decode_ref(codes, cb)))


def test_pq_unaligned_rows_take_the_general_path(be, oracle):
    x, cb = _data(3, 1000, 64, 8)
    buf = torch.zeros(1000 * 64 + 4, device=be.device)
    view = buf[1:1 + 1000 * 64].view(1000, 64)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    cbd = be._f32(cb)
    got = be.pq_encode(view, cbd, want_dist=True)
    _check(got, pq_encode_ref(oracle, x, cb), "offset by one float")
    aligned = be.pq_encode(x, cbd, want_dist=True)
    assert torch.equal(got[0], aligned[0]) and torch.equal(got[1].view(torch.int32), aligned[1].view(torch.int32))


def test_pq_argument_errors_and_empty_call(be):
    AT_E_INVALID = -1
    vp = ctypes.c_void_p
    x, cb = be.zeros((32, 64)), be.zeros((8, 256, 8))
    codes, out = be.empty((32, 8), torch.uint8), be.empty((32, 64))
    h = be.ctx.handle
    enc, dec = be.lib.at_pq_encode_f32, be.lib.at_pq_decode_f32
    px, pc, pk, po = vp(x.data_ptr()), vp(cb.data_ptr()), vp(codes.data_ptr()), vp(out.data_ptr())
    assert enc(h, px, 32, 64, 8, 256, pc, pk, None, None, None) == 0
    assert dec(h, pk, 32, 64, 8, 256, pc, po, None) == 0
    torch.cuda.synchronize(be.device)
    assert enc(h, None, 0, 64, 8, 256, None, None, None, None, None) == 0       # n == 0: no pointer is touched
    assert dec(h, None, 0, 64, 8, 256, None, None, None) == 0
    cases = [(None, px, 32, 64, 8, 256, pc, pk), (h, px, 32, 64, 7, 256, pc, pk), (h, px, 32, 64, 8, 0, pc, pk),
             (h, px, 32, 64, 8, 257, pc, pk), (h, px, -1, 64, 8, 256, pc, pk), (h, px, 32, 0, 8, 256, pc, pk),
             (h, px, 32, 64, 0, 256, pc, pk), (h, None, 32, 64, 8, 256, pc, pk), (h, px, 32, 64, 8, 256, None, pk),
             (h, px, 32, 64, 8, 256, pc, None)]
    for a in cases:
        assert enc(*a, None, None, None) == AT_E_INVALID, a
        assert b"at_pq_encode_f32" in be.lib.at_last_error()
    for a in [(None, pk, 32, 64, 8, 256, pc, po), (h, pk, 32, 64, 7, 256, pc, po), (h, pk, 32, 64, 8, 300, pc, po),
              (h, None, 32, 64, 8, 256, pc, po), (h, pk, 32, 64, 8, 256, None, po), (h, pk, 32, 64, 8, 256, pc, None)]:
        assert dec(*a, None) == AT_E_INVALID, a
        assert b"at_pq_decode_f32" in be.lib.at_last_error()
    with pytest.raises(ValueError):
        be.pq_encode(x, be.zeros((8, 256, 4)))
    got = be.pq_encode(be.zeros((0, 64)), cb, want_dist=True)
    assert tuple(got[0].shape) == (0, 8) and tuple(got[1].shape) == (0, 8) and int(got[2].item()) == 0


def test_pq_without_distances_and_two_streams_at_once(be, oracle):
    x1, c1 = _data(11, 20000, 64, 8)
    x2, c2 = _data(12, 5000, 128, 16)
    t = [be._f32(a) for a in (x1, c1, x2, c2)]
    want = [be.pq_encode(t[0], t[1], want_dist=True), be.pq_encode(t[2], t[3], want_dist=True)]
    _check(want[0], pq_encode_ref(oracle, x1, c1), "stream 1 shape")
    _check(want[1], pq_encode_ref(oracle, x2, c2), "stream 2 shape")
    codes, dist, bad = be.pq_encode(t[0], t[1])
    assert dist is None and torch.equal(codes, want[0][0]) and int(bad.item()) == 0
    torch.cuda.synchronize(be.device)
    s1, s2 = torch.cuda.Stream(be.device), torch.cuda.Stream(be.device)
    s1.wait_stream(torch.cuda.current_stream(be.device))
    s2.wait_stream(torch.cuda.current_stream(be.device))
    with torch.cuda.stream(s1):
        r1 = be.pq_encode(t[0], t[1], want_dist=True)
        r3 = be.pq_encode(t[0], t[1], want_dist=True)
    with torch.cuda.stream(s2):
        r2 = be.pq_encode(t[2], t[3], want_dist=True)
        r4 = be.pq_encode(t[2], t[3], want_dist=True)
    torch.cuda.synchronize(be.device)
    for got, ref in zip((r1, r2, r3, r4), (want[0], want[1], want[0], want[1])):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))


def test_product_quantizer_call_forms(be, oracle):
    from audio_tokens_amd.ops import ProductQuantizer
    x, cb = _data(9, 3000, 64, 8)
    cr, dr, _ = pq_encode_ref(oracle, x, cb)
    pq = ProductQuantizer(64, 8, backend=be)
    with pytest.raises(RuntimeError, match="not trained"):
        pq.compute_codes(x)
    pq.set_centroids(cb)
    codes, dist = pq.compute_codes(x, return_distances=True)                  # host in, numpy out
    assert isinstance(codes, np.ndarray) and codes.dtype == np.uint8 and dist.dtype == np.float32
    assert np.array_equal(codes, cr) and np.array_equal(bits(dist), bits(dr))
    xd = torch.from_numpy(x).to(be.device)
    codes_d = pq.compute_codes(xd)                                            # device in, device out
    assert codes_d.device == xd.device and codes_d.dtype == torch.uint8 and np.array_equal(_np(codes_d), cr)
    assert np.array_equal(pq.compute_codes(x.astype(np.float64)), cr)         # float64: converted to float32 first
    wide = torch.zeros((3000, 128), device=be.device)
    wide[:, ::2] = xd
    assert np.array_equal(_np(pq.compute_codes(wide[:, ::2])), cr)            # strided device view
    out = pq.decode(codes)                                                    # decode: host and device, round trip
    assert isinstance(out, np.ndarray) and np.array_equal(bits(out), bits(pq_decode_ref(cr, cb)))
    out_d = pq.decode(codes_d)
    assert out_d.device == xd.device and np.array_equal(bits(_np(out_d)), bits(out))
    again = pq.compute_codes(out_d, return_distances=True)                    # a decoded row is on its own words
    assert bool((again[1] == 0).all()) and np.array_equal(bits(_np(pq.decode(again[0]))), bits(out))
    bad = x.copy()
    bad[5, 9] = np.nan
    with pytest.raises(RuntimeError, match="input contains NaN's or Inf's"):
        pq.compute_codes(bad)
    got = pq.compute_codes(bad, check_finite=False)
    assert got[5, 1] == 0 and np.array_equal(np.delete(got, 5, 0), np.delete(cr, 5, 0))
    pq12 = ProductQuantizer(12, 4, backend=be)                                # scalar decode
    x12, cb12 = _data(10, 500, 12, 4)
    pq12.set_centroids(cb12)
    c12 = pq12.compute_codes(x12)
    assert np.array_equal(c12, pq_encode_ref(oracle, x12, cb12)[0])
    assert np.array_equal(bits(pq12.decode(c12)), bits(pq_decode_ref(c12, cb12)))


def test_pq_large_against_the_assign_composition(be):
    """n = 2^18, d = 64, M = 8: the fused call against one be.assign per contiguous slice, on the device."""
    n, d, M, dsub = 1 << 18, 64, 8, 8
    g = torch.Generator(device=be.device).manual_seed(4)
    cb = torch.randn(M, 256, dsub, device=be.device, generator=g)
    pick = torch.randint(0, 256, (n, M), device=be.device, generator=g)
    x = torch.cat([cb[m][pick[:, m]] for m in range(M)], 1) + 0.3 * torch.randn(n, d, device=be.device, generator=g)
    x = x.contiguous()
    codes, dist, bad = be.pq_encode(x, cb, want_dist=True)
    assert int(bad.item()) == 0
    for m in range(M):
        ids, dis = be.assign(x[:, m * dsub:(m + 1) * dsub].contiguous(), cb[m])
        assert torch.equal(codes[:, m].to(torch.int64), ids), m
        assert torch.equal(dist[:, m].contiguous().view(torch.int32), dis.view(torch.int32)), m
    out = be.pq_decode(codes, cb)
    for m in range(M):
        assert torch.equal(out[:, m * dsub:(m + 1) * dsub], cb[m][codes[:, m].to(torch.int64)])


def test_product_quantizer_train_on_the_device(be):
    from audio_tokens_amd.ops import Kmeans, ProductQuantizer
    rng = np.random.default_rng(8)
    x = rng.standard_normal((3000, 16)).astype(np.float32)
    pq = ProductQuantizer(16, 2, niter=4, backend=be)
    pq.train(x)
    assert pq.is_trained and pq.centroids.shape == (2, 256, 8)
    xd = be._f32(x)
    for m in range(2):
        km = Kmeans(8, 256, niter=4, seed=1234, backend=be)
        km.train(xd[:, 8 * m:8 * m + 8].contiguous())
        assert np.array_equal(bits(pq.centroids[m]), bits(km.centroids)), m
    codes = pq.compute_codes(x)
    assert codes.shape == (3000, 2) and len(np.unique(codes)) > 100
