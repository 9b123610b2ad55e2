"""ops.IndexPQ / HipBackend.pq_search / at_pq_search_f32 on the MI355X, bit for bit against tests/pq_search_ref.py (the
oracle's direct-form tables, float32 gathers added in ascending m, knn_ref.select) on every row of every case.  The seam
positions (queries per workgroup, rows per slab, queries per chunk) come from at_pq_search_limits."""
import ctypes

import numpy as np
import pytest
import torch

from pq_search_ref import pq_distances, pq_search_ref, pq_tables
from knn_ref import select

pytestmark = pytest.mark.gpu

# (d, M): dsub from 1 to 16, odd M (code rows at odd byte offsets: byte loads), M % 4, 8, 16 == 0 (4-, 8-, 16-byte
# loads), the largest table (M = 64: two queries per workgroup), the largest LDS request (M = 32: the last M with four
# queries per workgroup, 144 KiB) and two queries per workgroup with 8- and 4-byte loads (M = 40, M = 36)
SHAPES = [(8, 1), (8, 2), (16, 2), (64, 8), (64, 16), (128, 16), (64, 64), (24, 3), (12, 4), (15, 3), (64, 32), (80, 40),
          (36, 36)]
NTOTALS = [1, 5, 127, 128, 129, 1000]
KS = [1, 2, 10, 32, 33, 128]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _limits(be, M, ntotal, k):
    return be.pq_search_limits(M, ntotal, k)


def _check(got, ref, label=""):
    """got: (ids, dist) of be.pq_search; ref: (D, I) of the reference."""
    ids, dist = _np(got[0]), _np(got[1])
    D, I = ref
    assert ids.dtype == np.int64 and dist.dtype == np.float32 and ids.shape == I.shape and dist.shape == D.shape, label
    wrong = np.argwhere((ids != I) | (bits(dist) != bits(D)))
    assert wrong.size == 0, (label, len(wrong), wrong[:5], ids[tuple(wrong[0])], I[tuple(wrong[0])],
                             dist[tuple(wrong[0])], D[tuple(wrong[0])])


def _data(seed, n, d, M, ntotal, ksub=256):
    """Random codebooks and codes; a third of the queries sit close to a stored row."""
    rng = np.random.default_rng(seed)
    dsub = d // M
    cb = rng.standard_normal((M, ksub, dsub)).astype(np.float32)
    codes = rng.integers(0, ksub, (ntotal, M)).astype(np.uint8)
    x = rng.standard_normal((n, d)).astype(np.float32)
    for i in range(0, n, 3):
        r = codes[rng.integers(0, ntotal)]
        near = np.concatenate([cb[m][r[m]] for m in range(M)])
        x[i] = (near + np.float32(0.05) * x[i]).astype(np.float32)
    return x, cb, codes


@pytest.mark.parametrize("d,M", SHAPES)
def test_grid_bit_exact(be, oracle, d, M):
    qb = _limits(be, M, 1000, 1)["queries_per_block"]
    ns = sorted({1, 3, qb - 1, qb, qb + 1, 33})
    x, cb, codes = _data(d * 7 + M, 33, d, M, 1000)
    T = pq_tables(oracle, x, cb)                   # a query's table does not depend on the call: prefixes share it
    dis, ok = pq_distances(T, codes)
    cbd, xd, cd = be._f32(cb), be._f32(x), be.from_host(codes)
    for n in ns:
        for ntotal in NTOTALS:
            for k in KS:                           # (M = 64 meets k = 128 here, as every other pair does)
                got = be.pq_search(xd[:n], cbd, cd[:ntotal], k)
                _check(got, select(dis[:n, :ntotal], ok[:n, :ntotal], k), (d, M, n, ntotal, k))


def test_slab_seams(be, oracle):
    d, M = 8, 2
    slab = _limits(be, M, 1, 1)["slab_rows"]
    x, cb, codes = _data(3, 5, d, M, 2 * slab + 7)
    T = pq_tables(oracle, x, cb)
    dis, ok = pq_distances(T, codes)
    cbd, xd, cd = be._f32(cb), be._f32(x), be.from_host(codes)
    for ntotal in (slab - 1, slab, slab + 1, 2 * slab + 7):
        for k in (1, 10, 128):
            _check(be.pq_search(xd, cbd, cd[:ntotal], k), select(dis[:, :ntotal], ok[:, :ntotal], k), (ntotal, k))


def test_query_chunk_seam(be, oracle):
    """One below, at and one above the number of queries whose lists fill the workspace budget.  The queries are 40
    distinct rows repeated (a query's answer does not depend on the others), so every row has its reference."""
    d, M, k = 8, 2, 128
    slab = _limits(be, M, 1, 1)["slab_rows"]
    ntotal = 2 * slab + 7                          # three slabs: the chunk is a third of what one slab would allow
    lim = _limits(be, M, ntotal, k)
    chunk = lim["queries_per_chunk"]
    assert chunk % lim["queries_per_block"] == 0 and 1000 < chunk < 200000
    x, cb, codes = _data(5, 40, d, M, ntotal)
    D, I = pq_search_ref(oracle, x, cb, codes, k)
    cbd, cd = be._f32(cb), be.from_host(codes)
    reps = (chunk + 1 + 39) // 40
    xd = be._f32(np.tile(x, (reps, 1)))
    D, I = np.tile(D, (reps, 1)), np.tile(I, (reps, 1))
    for n in (chunk - 1, chunk, chunk + 1):
        _check(be.pq_search(xd[:n], cbd, cd, k), (D[:n], I[:n]), n)


def test_query_chunk_cap_of_the_merge_grid(be, oracle):
    """A small database and k = 1 make the lists of a query 8 bytes: the budget alone would allow 2^25 queries per chunk,
    more workgroups of 256 threads than one launch of the merge may have.  The chunk stops at 2^24 - 4; a call just
    above it takes two chunks."""
    d, M, k, ntotal = 8, 1, 1, 5
    chunk = _limits(be, M, ntotal, k)["queries_per_chunk"]
    assert chunk == (1 << 24) - 4 and chunk * 256 < (1 << 32)
    x, cb, codes = _data(6, 40, d, M, ntotal)
    D, I = pq_search_ref(oracle, x, cb, codes, k)
    n = chunk + 5
    reps = (n + 39) // 40
    xd = be._f32(x).repeat(reps, 1)[:n].contiguous()
    ids, dist = be.pq_search(xd, cb, codes, k)
    want_i = be.from_host(I).repeat(reps, 1)[:n]
    want_d = be.from_host(D).repeat(reps, 1)[:n]
    assert torch.equal(ids, want_i) and torch.equal(dist.view(torch.int32), want_d.contiguous().view(torch.int32))


def test_ties_across_a_slab_seam(be, oracle):
    d, M = 8, 2
    slab = _limits(be, M, 1, 1)["slab_rows"]
    x, cb, seven = _data(8, 6, d, M, 7)
    assert len({tuple(r) for r in seven}) == 7
    ntotal = slab + 140
    codes = np.tile(seven, (ntotal // 7 + 1, 1))[:ntotal]    # every tie group has members on both sides of the seam
    T = pq_tables(oracle, x, cb)
    cbd, xd = be._f32(cb), be._f32(x)
    dis, ok = pq_distances(T, codes)
    for k in (1, 39, 40, 41, 128):
        ref = select(dis, ok, k)
        _check(be.pq_search(xd, cbd, codes, k), ref, k)
        for i in range(6):                                   # the construction: the lowest ids of the nearest code row
            assert np.array_equal(ref[1][i], np.flatnonzero(dis[i] == dis[i].min())[:k])
    # a tie group that straddles the seam with few members on the low side: 20 equal rows at the end of slab 0, 20 at
    # the start of slab 1, every other row far away -- k = 30 takes all of the former and the lowest 10 of the latter
    far = np.array([np.argmax(T[0, m]) for m in range(M)], np.uint8)
    near = np.array([np.argmin(T[0, m]) for m in range(M)], np.uint8)
    codes = np.tile(far, (ntotal, 1))
    codes[slab - 20:slab + 20] = near
    dis, ok = pq_distances(T, codes)
    for k in (19, 20, 21, 30, 40, 41, 128):
        ref = select(dis, ok, k)
        _check(be.pq_search(xd, cbd, codes, k), ref, ("straddle", k))
        assert np.array_equal(ref[1][0, :min(k, 40)], np.arange(slab - 20, slab + 20)[:k])


def test_equal_words_and_queries_on_and_between_words(be, oracle):
    for d, M in ((64, 8), (12, 4), (15, 3)):
        dsub = d // M
        rng = np.random.default_rng(d)
        cb = rng.standard_normal((M, 256, dsub)).astype(np.float32)
        cb[:, 128:] = cb[:, :128]                            # word j equals word j + 128: other codes, the same distance
        codes = rng.integers(0, 256, (3000, M)).astype(np.uint8)
        codes[1500:] = codes[:1500] ^ 128                    # row r + 1500 ties with row r for every query
        a, b = codes[rng.integers(0, 3000, 12)], codes[rng.integers(0, 3000, 12)]
        on = np.stack([np.concatenate([cb[m][r[m]] for m in range(M)]) for r in a])
        other = np.stack([np.concatenate([cb[m][r[m]] for m in range(M)]) for r in b])
        x = np.concatenate([on, (on * np.float32(0.5) + other * np.float32(0.5)).astype(np.float32)])
        T = pq_tables(oracle, x, cb)
        dis, ok = pq_distances(T, codes)
        assert np.all(dis[:12].min(1) == 0)                  # a query on a stored row is at distance +0
        assert np.array_equal(bits(dis[:, :1500]), bits(dis[:, 1500:]))
        for k in (1, 2, 7, 128):
            ref = select(dis, ok, k)
            _check(be.pq_search(x, cb, codes, k), ref, (d, M, k))
            if k >= 2:                                       # the best row ties with its twin: the lower id leads
                assert np.all(ref[1][:, 0] < 1500) and np.array_equal(bits(ref[0][:, 0]), bits(ref[0][:, 1]))


def test_non_finite_queries_and_words(be, oracle):
    d, M = 64, 8
    x, cb, codes = _data(12, 12, d, M, 700)
    clean = pq_search_ref(oracle, x, cb, codes, 10)
    x[2, 17] = np.nan                                        # sub-space 2
    x[4, 63] = np.inf                                        # sub-space 7
    x[6, 0] = -np.inf                                        # sub-space 0
    x[8, 40] = 3e38                                          # sub-space 5: (x - c)^2 overflows
    ref = pq_search_ref(oracle, x, cb, codes, 10)
    for i in (2, 4, 6, 8):
        assert np.all(ref[1][i] == -1) and np.all(np.isposinf(ref[0][i]))
    rest = [i for i in range(12) if i not in (2, 4, 6, 8)]
    assert np.array_equal(ref[1][rest], clean[1][rest]) and np.array_equal(bits(ref[0][rest]), bits(clean[0][rest]))
    _check(be.pq_search(x, cb, codes, 10), ref, "queries")
    _check(be.pq_search(x[:3], cb, codes, 128), pq_search_ref(oracle, x[:3], cb, codes, 128), "queries, k = 128")

    x, cb, codes = _data(13, 7, d, M, 700)
    cb[3, 77, 5] = np.nan                                    # the rows that use word 77 of sub-space 3 are never listed
    codes[::9, 3] = 77
    uses = set(np.flatnonzero(codes[:, 3] == 77).tolist())
    got = be.pq_search(x, cb, codes, 128)
    _check(got, pq_search_ref(oracle, x, cb, codes, 128), "word")
    wide = be.pq_search(np.tile(x, (1, 1)), cb, codes[:120], 128)      # k > rows left: every other row is listed
    for i in range(7):
        listed = set(_np(wide[0])[i].tolist()) - {-1}
        assert listed == set(range(120)) - uses
    assert not (set(_np(got[0]).ravel().tolist()) & uses)


@pytest.mark.parametrize("ksub", [1, 7, 255])
def test_small_codebooks_and_codes_outside_them(be, oracle, ksub):
    for d, M in ((64, 8), (15, 3)):
        x, cb, codes = _data(ksub + d, 9, d, M, 400, ksub)
        planted = [3, 64, 65, 399]
        codes[planted, [0, M - 1, 1, 0]] = [ksub, 255, ksub, 255]
        ref = pq_search_ref(oracle, x, cb, codes, 128)
        got = be.pq_search(x, cb, codes, 128)
        _check(got, ref, (ksub, d, M))
        assert not (set(_np(got[0]).ravel().tolist()) & set(planted))
        _check(be.pq_search(x, cb, codes, 3), pq_search_ref(oracle, x, cb, codes, 3), (ksub, d, M, 3))


def test_offset_pointers_and_no_distances(be, oracle):
    d, M, ntotal = 64, 16, 900
    x, cb, codes = _data(31, 10, d, M, ntotal)
    ref = pq_search_ref(oracle, x, cb, codes, 20)
    cbd = be._f32(cb)
    buf = torch.zeros(10 * d + 4, device=be.device)
    xv = buf[1:1 + 10 * d].view(10, d)
    xv.copy_(torch.from_numpy(x))
    assert xv.data_ptr() % 16 == 4 and xv.is_contiguous()
    _check(be.pq_search(xv, cbd, codes, 20), ref, "x offset by one float")
    raw = torch.zeros(ntotal * M + 16, dtype=torch.uint8, device=be.device)
    for off in (1, 4, 8):                                    # byte loads, 4-byte loads, 8-byte loads of the same rows
        cv = raw[off:off + ntotal * M].view(ntotal, M)
        cv.copy_(torch.from_numpy(codes))
        assert cv.data_ptr() % 16 == off and cv.is_contiguous()
        _check(be.pq_search(x, cbd, cv, 20), ref, ("codes offset", off))
    ids, dist = be.pq_search(x, cbd, codes, 20, want_dist=False)
    assert dist is None and np.array_equal(_np(ids), ref[1])


def test_column_zero_does_not_depend_on_k(be):
    x, cb, codes = _data(17, 64, 64, 8, 100000)
    cbd, cd = be._f32(cb), be.from_host(codes)
    one, many = be.pq_search(x, cbd, cd, 1), be.pq_search(x, cbd, cd, 128)
    assert torch.equal(one[0][:, 0], many[0][:, 0]) and torch.equal(one[1][:, 0].view(torch.int32),
                                                                    many[1][:, 0].contiguous().view(torch.int32))
    assert bool((many[1][:, 1:] >= many[1][:, :-1]).all()) and bool((many[0] >= 0).all())


def test_argument_errors_and_empty_calls(be):
    AT_E_INVALID = -1
    vp = ctypes.c_void_p
    x, cb = be.zeros((8, 64)), be.zeros((8, 256, 8))
    codes = be.zeros((100, 8), torch.uint8)
    ids, dist = be.empty((8, 5), torch.int64), be.empty((8, 5))
    h = be.ctx.handle
    fn = be.lib.at_pq_search_f32
    px, pc, pk, pi, pd = (vp(t.data_ptr()) for t in (x, cb, codes, ids, dist))
    assert fn(h, px, 8, 64, 8, 256, pc, pk, 100, 5, pi, pd, None) == 0
    assert fn(h, px, 8, 64, 8, 256, pc, pk, 100, 5, pi, None, None) == 0
    torch.cuda.synchronize(be.device)
    assert bool((dist == 0).all()) and _np(ids).tolist() == [list(range(5))] * 8       # all ties: the lowest ids
    assert fn(h, None, 0, 64, 8, 256, None, None, 100, 5, None, None, None) == 0        # n == 0: no pointer is touched
    ids.fill_(7)
    dist.fill_(7)
    assert fn(h, px, 8, 64, 8, 256, pc, None, 0, 5, pi, pd, None) == 0                  # ntotal == 0: (-1, +inf)
    torch.cuda.synchronize(be.device)
    assert bool((ids == -1).all()) and bool(torch.isposinf(dist).all())
    cases = [(None, px, 8, 64, 8, 256, pc, pk, 100, 5, pi, pd), (h, px, -1, 64, 8, 256, pc, pk, 100, 5, pi, pd),
             (h, px, 8, 0, 8, 256, pc, pk, 100, 5, pi, pd), (h, px, 8, 64, 0, 256, pc, pk, 100, 5, pi, pd),
             (h, px, 8, 64, 7, 256, pc, pk, 100, 5, pi, pd), (h, px, 8, 65, 65, 256, pc, pk, 100, 5, pi, pd),
             (h, px, 8, 64, 8, 0, pc, pk, 100, 5, pi, pd), (h, px, 8, 64, 8, 257, pc, pk, 100, 5, pi, pd),
             (h, px, 8, 64, 8, 256, pc, pk, -1, 5, pi, pd), (h, px, 8, 64, 8, 256, pc, pk, 1 << 31, 5, pi, pd),
             (h, px, 8, 64, 8, 256, pc, pk, 100, 0, pi, pd), (h, px, 8, 64, 8, 256, pc, pk, 100, 129, pi, pd),
             (h, None, 8, 64, 8, 256, pc, pk, 100, 5, pi, pd), (h, px, 8, 64, 8, 256, None, pk, 100, 5, pi, pd),
             (h, px, 8, 64, 8, 256, pc, None, 100, 5, pi, pd), (h, px, 8, 64, 8, 256, pc, pk, 100, 5, None, pd)]
    for a in cases:
        assert fn(*a, None) == AT_E_INVALID, a
        assert b"at_pq_search_f32" in be.lib.at_last_error()
    with pytest.raises(ValueError):
        be.pq_search(x, be.zeros((8, 256, 4)), codes, 5)
    with pytest.raises(RuntimeError, match="at least 1"):
        be.pq_search(x, cb, codes, 0)
    got = be.pq_search(be.zeros((0, 64)), cb, codes, 5)
    assert tuple(got[0].shape) == (0, 5) and tuple(got[1].shape) == (0, 5)
    got = be.pq_search(x, cb, be.zeros((0, 8), torch.uint8), 5)
    assert bool((got[0] == -1).all()) and bool(torch.isposinf(got[1]).all())
    lim = be.pq_search_limits(8, 100, 5)
    assert lim["queries_per_block"] == 4 and be.pq_search_limits(33, 100, 5)["queries_per_block"] == 2
    assert be.lib.at_pq_search_limits(None, None, None, 65, 100, 5) == AT_E_INVALID


def test_two_streams_at_once(be, oracle):
    x1, c1, k1 = _data(41, 64, 64, 8, 200000)
    x2, c2, k2 = _data(42, 48, 128, 16, 150000)
    t = [be._f32(x1), be._f32(c1), be.from_host(k1), be._f32(x2), be._f32(c2), be.from_host(k2)]
    want = [be.pq_search(t[0], t[1], t[2], 100), be.pq_search(t[3], t[4], t[5], 7)]
    _check((want[0][0][:5], want[0][1][:5]), pq_search_ref(oracle, x1[:5], c1, k1, 100), "stream 1 shape")
    _check((want[1][0][:5], want[1][1][:5]), pq_search_ref(oracle, x2[:5], c2, k2, 7), "stream 2 shape")
    torch.cuda.synchronize(be.device)
    s1, s2 = torch.cuda.Stream(be.device), torch.cuda.Stream(be.device)
    s1.wait_stream(torch.cuda.current_stream(be.device))
    s2.wait_stream(torch.cuda.current_stream(be.device))
    with torch.cuda.stream(s1):
        r1 = be.pq_search(t[0], t[1], t[2], 100)
        r3 = be.pq_search(t[0], t[1], t[2], 100)
    with torch.cuda.stream(s2):
        r2 = be.pq_search(t[3], t[4], t[5], 7)
        r4 = be.pq_search(t[3], t[4], t[5], 7)
    torch.cuda.synchronize(be.device)
    for got, ref in zip((r1, r2, r3, r4), (want[0], want[1], want[0], want[1])):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))


def test_index_pq_end_to_end(be, oracle):
    from audio_tokens_amd.ops import IndexPQ
    rng = np.random.default_rng(6)
    x = rng.standard_normal((6000, 64)).astype(np.float32)
    q = (x[rng.integers(0, 6000, 20)] + np.float32(0.1) * rng.standard_normal((20, 64))).astype(np.float32)
    index = IndexPQ(64, 8, niter=3, backend=be)
    with pytest.raises(RuntimeError, match="not trained"):
        index.search(q, 3)
    index.train(x)
    assert index.is_trained and index.ntotal == 0
    D0, I0 = index.search(q, 4)
    assert np.all(I0 == -1) and np.all(np.isposinf(D0))
    index.add(x[:2500])
    index.add(torch.from_numpy(x[2500:]).to(be.device))
    assert index.ntotal == 6000 and index.codes.device == be.device and index.codes.dtype == torch.uint8
    codes = _np(index.codes)
    assert np.array_equal(codes, index.pq.compute_codes(x))
    Dr, Ir = pq_search_ref(oracle, q, index.pq.centroids, codes, 10)
    D, I = index.search(q, 10)                                             # host in, numpy out
    assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray)
    assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))
    qd = torch.from_numpy(q).to(be.device)
    Dd, Id = index.search(qd, 10)                                          # device in, device out
    assert Dd.device == qd.device and Id.dtype == torch.int64 and Dd.dtype == torch.float32
    assert np.array_equal(_np(Id), Ir) and np.array_equal(bits(_np(Dd)), bits(Dr))
    with pytest.raises(NotImplementedError, match="128"):
        index.search(q, 129)
    dec = index.pq.decode(codes)
    assert np.array_equal(bits(index.reconstruct_n(100, 50)), bits(dec[100:150]))
    assert np.array_equal(bits(index.reconstruct(5999)), bits(dec[5999]))
    index.reset()
    assert index.ntotal == 0 and index.is_trained and np.all(index.search(q, 2)[1] == -1)
    index.add_codes(codes[:1000])
    index.add_codes(index.pq.compute_codes(qd.new_tensor(x[1000:])))
    assert index.ntotal == 6000
    D2, I2 = index.search(q, 10)
    assert np.array_equal(I2, Ir) and np.array_equal(bits(D2), bits(Dr))
