"""IndexFlatL2.search(x, k) / at_knn_f32 on the MI355X, bit for bit against tests/knn_ref.py (the oracle's distances,
selected per row in (dis, id) order) and against the k = 1 paths."""
import numpy as np
import pytest
import torch

from knn_ref import knn_ref

pytestmark = pytest.mark.gpu

K_FUSED = 32   # largest k of the fused sweep (csrc/knn.hip)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _unit(rng, n, d, oracle):
    return oracle.l2norm_rows(rng.standard_normal((n, d)).astype(np.float32))


def _check(D, I, Dr, Ir, label=""):
    D, I = np.asarray(D), np.asarray(I)
    assert D.shape == Dr.shape and I.shape == Ir.shape, label
    bad = np.nonzero((I != Ir).any(1) | (bits(D) != bits(Dr)).any(1))[0]
    assert bad.size == 0, (label, bad[:5], I[bad[:1]], Ir[bad[:1]], D[bad[:1]], Dr[bad[:1]])


def _data(seed, n, d, kc, oracle):
    rng = np.random.default_rng(seed)
    c = _unit(rng, kc, d, oracle)
    if kc > 2:
        c[kc // 2] = c[1]                                        # an exact duplicate
    x = _unit(rng, n, d, oracle)
    if n > 3:
        x[: n // 4] = (c[rng.integers(0, kc, n // 4)] + np.float32(0.01) * x[: n // 4]).astype(np.float32)
        x[1] = c[min(1, kc - 1)]                                 # a row on the duplicated centroid
    return x, c


# every value of d, k_c, k and n appears; k_c = 8192 only at d <= 128 (the reference costs n * k_c * d fmas)
GRID = [
    (64, 8192, 2, 4097), (64, 8192, 33, 4097), (128, 8192, K_FUSED, 4097), (128, 500, 16, 4097),
    (64, 256, 5, 20), (64, 7, 7, 4097), (8, 7, 10, 4097), (50, 500, 100, 4097), (640, 256, 33, 20),
    (1280, 7, 2, 4097), (1280, 256, 256, 19), (640, 500, 5, 1), (64, 1, 2, 4097), (128, 1, 4, 19),
    (50, 256, 16, 20), (8, 500, K_FUSED, 19), (640, 500, K_FUSED + 1, 4097), (128, 256, 100, 20),
    (64, 500, 503, 20), (640, 7, 16, 4097),
    # the list lengths the rows above leave out at a width, at the edges of the sweep: a second workgroup with one live
    # row, a second tile with one real centroid, a second chunk of one 16-byte piece (d = 68), three chunks (d = 192)
    (64, 129, 16, 129), (128, 129, 3, 129), (128, 300, 8, 129), (68, 129, 8, 129), (192, 129, K_FUSED, 129),
]


@pytest.mark.parametrize("d,kc,k,n", GRID)
def test_knn_grid_bit_exact(be, oracle, d, kc, k, n):
    x, c = _data(d * 7 + kc + k + n, n, d, kc, oracle)
    Dr, Ir = knn_ref(oracle, x, c, k)
    I, D = be.knn(x, c, k)
    _check(D.cpu().numpy(), I.cpu().numpy(), Dr, Ir, (d, kc, k, n))
    ids, dis = be.assign(x, c)                                   # column 0 is the k = 1 answer
    assert np.array_equal(I[:, 0].cpu().numpy(), ids.cpu().numpy())
    assert np.array_equal(bits(D[:, 0].cpu().numpy()), bits(dis.cpu().numpy()))


def test_knn_without_distances(be, oracle):
    x, c = _data(1, 300, 64, 256, oracle)
    for k in (8, 40):
        I, D = be.knn(x, c, k, want_dist=False)
        assert D is None
        assert torch.equal(I, be.knn(x, c, k)[0])


def test_knn_near_ties_and_bad_values(be, oracle):
    """tests/test_gpu_ops.py::test_filter_near_ties_and_bad_values's construction: exact midpoints, duplicated
    centroids, rows equal to centroids, an out-of-fp16-range row and centroid, a NaN row."""
    rng = np.random.default_rng(23)
    n, d, kc = 3000, 64, 1024
    c = _unit(rng, kc, d, oracle)
    c[700:720] = c[100:120]
    a, b = rng.integers(0, kc, n), rng.integers(0, kc, n)
    t = np.float32(0.5) + rng.choice([0.0, 1e-7, -1e-7, 1e-6, -1e-5, 1e-4, -1e-3], n).astype(np.float32)
    x = (c[a] * t[:, None] + c[b] * (np.float32(1) - t)[:, None] + 0.002 * rng.standard_normal((n, d))).astype(np.float32)
    x[:200] = (c[a[:200]] * np.float32(0.5) + c[b[:200]] * np.float32(0.5)).astype(np.float32)
    x[200:300] = c[rng.integers(0, kc, 100)]
    x[300:320] = c[100:120]                                       # rows on duplicated centroids
    for label in ("plain", "big_row", "big_centroid", "nan_row"):
        xx, cc = x.copy(), c.copy()
        if label == "big_row":
            xx[5, 3] = 70000.0
        if label == "big_centroid":
            cc[9, 1] = 40000.0
        if label == "nan_row":
            xx[7, 0] = np.nan
        for k in (8, K_FUSED + 8):
            Dr, Ir = knn_ref(oracle, xx, cc, k)
            I, D = be.knn(xx, cc, k)
            _check(D.cpu().numpy(), I.cpu().numpy(), Dr, Ir, (label, k))
        if label == "nan_row":
            assert np.all(Ir[7] == -1) and np.all(np.isposinf(Dr[7]))


@pytest.mark.parametrize("k", [8, 32])
def test_knn_large_against_search_1(be, oracle, k):
    """n = 2^21, k_c = 8192, d = 64: column 0 equals search(x, 1) (the filter path), every row is sorted under
    (dis, id), and 1024 sampled rows match the reference."""
    from audio_tokens_amd.ops import IndexFlatL2
    n, d, kc = 1 << 21, 64, 8192
    g = torch.Generator(device=be.device).manual_seed(k)
    c = torch.nn.functional.normalize(torch.randn(kc, d, device=be.device, generator=g), dim=1)
    pick = torch.randint(0, kc, (n,), device=be.device, generator=g)
    x = torch.nn.functional.normalize(c[pick] + 0.05 * torch.randn(n, d, device=be.device, generator=g), dim=1)
    index = IndexFlatL2(d, backend=be)
    index.add(c)
    D1, I1 = index.search(x, 1)
    D, I = index.search(x, k)
    assert D.shape == (n, k) and I.shape == (n, k) and D.device == x.device
    assert torch.equal(I[:, 0], I1[:, 0]) and torch.equal(D[:, 0].view(torch.int32), D1[:, 0].view(torch.int32))
    assert bool((I >= 0).all())
    dd, ii = D[:, 1:], I[:, 1:]
    assert bool(((dd > D[:, :-1]) | ((dd == D[:, :-1]) & (ii > I[:, :-1]))).all())
    rows = np.random.default_rng(k).choice(n, 1024, replace=False)
    Dr, Ir = knn_ref(oracle, x[rows].cpu().numpy(), c.cpu().numpy(), k)
    _check(D[rows].cpu().numpy(), I[rows].cpu().numpy(), Dr, Ir, k)


def test_search_host_device_and_conversions(be, oracle):
    from audio_tokens_amd.ops import IndexFlatL2
    x, c = _data(9, 3000, 64, 500, oracle)
    index = IndexFlatL2(64, backend=be)
    index.add(c)
    for k in (6, 50):
        Dr, Ir = knn_ref(oracle, x, c, k)
        D, I = index.search(x, k)                                  # host in, numpy out
        assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray)
        assert D.dtype == np.float32 and I.dtype == np.int64 and D.flags.c_contiguous
        _check(D, I, Dr, Ir, ("host", k))
        xd = torch.from_numpy(x).to(be.device)
        D, I = index.search(xd, k)                                 # device in, device out
        assert D.device == xd.device and I.device == xd.device
        _check(D.cpu().numpy(), I.cpu().numpy(), Dr, Ir, ("device", k))
        D, I = index.search(x.astype(np.float64), k)               # float64: converted to float32 first
        _check(D, I, Dr, Ir, ("float64", k))
        wide = torch.zeros((3000, 128), device=be.device)
        wide[:, ::2] = xd
        D, I = index.search(wide[:, ::2], k)                       # strided device view
        _check(D.cpu().numpy(), I.cpu().numpy(), Dr, Ir, ("strided", k))
        D1, I1 = index.search(x, 1)
        assert np.array_equal(I[:, 0].cpu().numpy(), I1[:, 0]) and np.array_equal(bits(D[:, 0].cpu().numpy()), bits(D1[:, 0]))


def test_knn_two_streams_at_once(be, oracle):
    x1, c1 = _data(11, 20000, 64, 2048, oracle)
    x2, c2 = _data(12, 5000, 128, 700, oracle)
    t = [torch.from_numpy(a).to(be.device) for a in (x1, c1, x2, c2)]
    want = [be.knn(t[0], t[1], 8), be.knn(t[2], t[3], 40), be.knn(t[0], t[1], 60), be.knn(t[2], t[3], 3)]
    torch.cuda.synchronize(be.device)
    s1, s2 = torch.cuda.Stream(be.device), torch.cuda.Stream(be.device)
    s1.wait_stream(torch.cuda.current_stream(be.device))
    s2.wait_stream(torch.cuda.current_stream(be.device))
    with torch.cuda.stream(s1):
        r1 = be.knn(t[0], t[1], 8)
        r3 = be.knn(t[0], t[1], 60)
    with torch.cuda.stream(s2):
        r2 = be.knn(t[2], t[3], 40)
        r4 = be.knn(t[2], t[3], 3)
    torch.cuda.synchronize(be.device)
    for got, ref in zip((r1, r2, r3, r4), want):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))


def test_search_empty_index_and_bad_k(be):
    from audio_tokens_amd import _lib
    from audio_tokens_amd.ops import IndexFlatL2
    index = IndexFlatL2(64, backend=be)
    x = np.ones((5, 64), np.float32)
    D, I = index.search(x, 4)
    assert D.shape == (5, 4) and np.all(np.isposinf(D)) and np.all(I == -1)
    index.add(np.eye(64, dtype=np.float32)[:10])
    for bad in (0, -1):
        with pytest.raises(RuntimeError):
            index.search(x, bad)
    xd, cd = be._f32(x), be._f32(np.eye(64, dtype=np.float32)[:10])
    ids = be.empty((5, 4), torch.int64)
    rc = be.lib.at_knn_f32(be.ctx.handle, _lib.ctypes.c_void_p(xd.data_ptr()), 5, 64,
                           _lib.ctypes.c_void_p(cd.data_ptr()), 10, 0, _lib.ctypes.c_void_p(ids.data_ptr()), None, None)
    assert rc < 0
