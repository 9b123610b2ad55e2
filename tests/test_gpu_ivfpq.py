"""ops.IndexIVFPQ / HipBackend.ivfpq_build / ivfpq_search / at_ivfpq_* on the MI355X, ids and distance bits against
tests/ivfpq_ref.py (the oracle's direct-form tables on the residual queries, knn_ref's probes and selection) on every row
of every case.  The reference costs M * ksub * ceil(pairs of a list / 19) oracle calls per list, so the many-pair cases run
at (d, M) = (8, 1) and (8, 2) or with ksub = 7, the wide shapes with a few queries; the seams (pairs per workgroup, rows
per group, queries per chunk) come from at_ivfpq_search_limits."""
import ctypes

import numpy as np
import pytest
import torch

from ivf_ref import check_ties, ivf_lists, ivf_probes, ivf_select
from ivfpq_ref import ivfpq_distances, ivfpq_encoder_input, ivfpq_search_ref
from pq_ref import pq_decode_ref, pq_encode_ref
from test_ivfpq_ref import TIE_CASES, TIE_KS, _brute_distances, tie_codes

pytestmark = pytest.mark.gpu

KS = (1, 2, 10, 32, 33, 128)
SHAPES = [(8, 1), (8, 2), (64, 8), (64, 16), (128, 16), (24, 3), (15, 3), (64, 32), (80, 40), (36, 36)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def _check(got, ref, label=""):
    """got: (D, I) of IndexIVFPQ.search; ref: (D, I) of the reference."""
    dist, ids = _np(got[0]), _np(got[1])
    D, I = ref
    assert ids.dtype == np.int64 and dist.dtype == np.float32 and ids.shape == I.shape and dist.shape == D.shape, label
    wrong = np.argwhere((ids != I) | (bits(dist) != bits(D)))
    assert wrong.size == 0, (label, len(wrong), wrong[:5], ids[tuple(wrong[0])], I[tuple(wrong[0])],
                             dist[tuple(wrong[0])], D[tuple(wrong[0])])


def _check_backend(got, ref, label=""):
    """got: (ids, dist) of be.ivfpq_search."""
    _check((got[1], got[0]), ref, label)


def _clustered(seed, d, M, nlist, ntotal, nq, ksub=256):
    """nlist centres, stored rows and queries scattered round them, and codebooks at the scale of the scatter."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    stored = (cent[rng.integers(0, nlist, ntotal)] + 0.7 * rng.standard_normal((ntotal, d))).astype(np.float32)
    x = (cent[rng.integers(0, nlist, nq)] + 0.7 * rng.standard_normal((nq, d))).astype(np.float32)
    cb = (0.7 * rng.standard_normal((M, ksub, d // M))).astype(np.float32)
    return x, stored, cent, cb


def _index(be, cent, cb, by_residual, nlist=None):
    from audio_tokens_amd.ops import IndexFlatL2, IndexIVFPQ
    d = cent.shape[1]
    quant = IndexFlatL2(d, backend=be)
    quant.add(cent)
    index = IndexIVFPQ(quant, d, nlist or cent.shape[0], cb.shape[0], by_residual=by_residual, backend=be)
    index.pq.set_centroids(cb)
    return index


def _limits(be, M, nprobe, k):
    return be.ivfpq_search_limits(M, nprobe, k)


def _grid_plan(d, M, by_residual):
    """(nlist, query counts) per shape: every (d, M) with both list counts where the reference can afford it."""
    if M * 256 <= 512:
        return [(7, (1, 3, 19, 20, 33)), (61, (1, 3, 19, 20, 33))]
    if not by_residual:                                           # one set of tables serves every list
        return [(7, (1, 3, 19, 20, 33)), (61, (3, 20))]
    if M * 256 <= 768:
        return [(7, (1, 3, 19, 20, 33)), (61, (3, 19))]
    if M * 256 <= 2048:
        return [(7, (1, 3, 19, 20, 33))]
    return [(7, (3, 19))]


@pytest.mark.parametrize("by_residual", [True, False])
@pytest.mark.parametrize("d,M", SHAPES)
def test_grid_bit_exact(be, oracle, d, M, by_residual):
    for nlist, ns in _grid_plan(d, M, by_residual):
        ntotal = 600
        x, stored, cent, cb = _clustered(1000 * d + 10 * M + nlist, d, M, nlist, ntotal, max(ns))
        lists = ivf_lists(oracle, stored, cent)
        assert np.all(lists >= 0)
        index = _index(be, cent, cb, by_residual)
        index.add(stored)
        codes = _np(index.codes)
        want, _, flag = pq_encode_ref(oracle, ivfpq_encoder_input(stored, lists, cent, by_residual), cb)
        assert not flag and np.array_equal(codes, want)           # the stored codes are the quantiser's for the residuals
        assert index.ntotal == ntotal and np.array_equal(index.list_sizes, np.bincount(lists, minlength=nlist))
        dis, ok = ivfpq_distances(oracle, x, cb, codes, lists, cent, by_residual)
        for n in ns:
            for nprobe in (1, 3, nlist, nlist + 5):
                probes = ivf_probes(oracle, x[:n], cent, nprobe)  # (n < 20: the direct form decides the probes)
                index.nprobe = nprobe
                for k in KS:
                    ref = ivf_select(dis[:n], ok[:n], lists, probes, k)
                    _check(index.search(x[:n], k), ref, (d, M, by_residual, nlist, n, nprobe, k))


@pytest.mark.parametrize("d,M", [(64, 8), (15, 3)])
def test_equals_index_pq_when_every_list_is_probed(be, d, M):
    from audio_tokens_amd.ops import IndexPQ
    nlist = 7
    x, stored, cent, cb = _clustered(5 + d, d, M, nlist, 3000, 70)
    index = _index(be, cent, cb, False)
    index.add(stored)
    assert int(index.list_sizes.sum()) == 3000                    # no stored row is unlisted
    flat = IndexPQ(d, M, backend=be)
    flat.pq.set_centroids(cb)
    flat.add_codes(index.codes)
    xd = be._f32(x)
    for nprobe in (nlist, nlist + 5):
        index.nprobe = nprobe
        for n in (1, 3, 19, 20, 70):                              # neither side has a rule keyed on n
            for k in KS:
                (D, I), (Df, If) = index.search(xd[:n], k), flat.search(xd[:n], k)
                assert torch.equal(I, If) and torch.equal(D.view(torch.int32), Df.view(torch.int32)), (n, k)


@pytest.mark.parametrize("by_residual", [True, False])
def test_constructed_lists_a_long_list_and_under_full_results(be, oracle, by_residual):
    d, M, k = 8, 2, 128
    sizes = [0, 1, 15, 16, 17, 255, 256, 257, 40, 1500]
    nlist, long_list, lonely = len(sizes), 9, 8
    rng = np.random.default_rng(78)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    cent[lonely] += 40.0                                          # far from every query: nobody probes this list
    cb = (0.7 * rng.standard_normal((M, 256, d // M))).astype(np.float32)
    group = _limits(be, M, 1, k)["rows_per_group"]
    assert sizes[2] == group - 1 and sizes[3] == group and sizes[4] == group + 1 and sizes[6] == 256
    x = (cent[np.arange(40) % 8] + 0.3 * rng.standard_normal((40, d))).astype(np.float32)
    x[0] = cent[long_list] + 0.1                                  # the query the long list is laid out for
    x[1:4] = cent[long_list] + 0.3 * rng.standard_normal((3, d)).astype(np.float32)
    # the long list: code rows at pairwise distinct distances from query 0, stored in DESCENDING order of that distance,
    # so every row is below the threshold when it arrives, the buffer fills in the first round and is cut mid-scan
    cand = np.unique(rng.integers(0, 256, (6000, M)).astype(np.uint8), axis=0)
    dq, okq = ivfpq_distances(oracle, x[:1], cb, cand, np.full(cand.shape[0], long_list), cent, by_residual)
    assert okq.all()
    _, pick = np.unique(dq[0], return_index=True)
    assert pick.size >= sizes[long_list]
    long_codes = cand[pick[:sizes[long_list]][::-1]]              # np.unique sorts ascending: reversed, descending
    given = np.concatenate([np.full(s, l, np.int64) for l, s in enumerate(sizes)])
    given = given[rng.permutation(given.size)]
    codes = rng.integers(0, 256, (given.size, M)).astype(np.uint8)
    codes[given == long_list] = long_codes                        # ascending id inside the list: descending distance
    image = be.ivfpq_build(torch.from_numpy(codes), torch.from_numpy(given), nlist)
    assert image["ngroups"] == given.size // group + nlist
    first = _np(image["first"])
    assert np.array_equal(np.diff(first), [(s + group - 1) // group for s in sizes])
    pos2id = _np(image["pos2id"])[:first[-1] * group]
    assert np.array_equal(np.sort(pos2id[pos2id >= 0]), np.arange(given.size))
    for l in range(nlist):                                        # ids ascend inside a list, pads behind them
        mine = pos2id[first[l] * group:first[l + 1] * group]
        assert np.array_equal(mine[:sizes[l]], np.flatnonzero(given == l)) and np.all(mine[sizes[l]:] == -1)
    assert np.array_equal(_np(image["codes"])[:first[-1] * group][pos2id >= 0], codes[pos2id[pos2id >= 0]])
    dis, ok = ivfpq_distances(oracle, x, cb, codes, given, cent, by_residual)
    mine = dis[0][given == long_list]
    assert ok[0][given == long_list].all() and np.all(np.diff(mine) < 0) and mine.size >= 1500
    cd, xd = be._f32(cent), be._f32(x)
    for nprobe in (1, 3):
        probes = ivf_probes(oracle, x, cent, nprobe)
        assert not np.any(probes == lonely) and all(np.any(probes == l) for l in range(8)) and probes[0, 0] == long_list
        got = be.ivfpq_search(xd, torch.from_numpy(probes), cd if by_residual else None, cb, image, k)
        D, I = ivf_select(dis, ok, given, probes, k)
        _check_backend(got, (D, I), nprobe)
        if nprobe == 1:                                           # queries of the short lists find fewer than k rows
            short = I[:, -1] == -1
            assert 0 < np.count_nonzero(short) < x.shape[0] and np.all(I[:4, -1] >= 0)
            assert np.all(np.isposinf(D[I == -1])) and np.all(np.isfinite(D[I >= 0]))
    nobody = np.full((5, 2), -1, np.int64)                        # probes that name no list, and an empty list alone
    nobody[3, 1] = 0
    got = be.ivfpq_search(xd[:5], torch.from_numpy(nobody), cd if by_residual else None, cb, image, 4)
    assert np.all(_np(got[0]) == -1) and np.all(np.isposinf(_np(got[1])))


@pytest.mark.parametrize("d,M", [(8, 2), (80, 40)])
@pytest.mark.parametrize("by_residual", [True, False])
def test_pair_block_seams(be, oracle, d, M, by_residual):
    nlist, k = 5, 10
    qb = _limits(be, M, 2, k)["pairs_per_block"]
    assert qb == (4 if M <= 32 else 2)
    x, stored, cent, cb = _clustered(9 + d, d, M, nlist, 200, 2 * qb + 1)
    lists = ivf_lists(oracle, stored, cent)
    codes, _, _ = pq_encode_ref(oracle, ivfpq_encoder_input(stored, lists, cent, by_residual), cb)
    image = be.ivfpq_build(torch.from_numpy(codes), torch.from_numpy(lists), nlist)
    assert np.count_nonzero(lists == 2) > k
    for n in (qb - 1, qb, qb + 1, 2 * qb + 1):
        probes = np.full((n, 2), 2, np.int64)                     # every query probes list 2 ...
        probes[:, 1] = -1
        if n > 1:
            probes[1::2, 1] = 4                                   # ... every other one list 4 as well; query 0 nothing else
        dis, ok = ivfpq_distances(oracle, x[:n], cb, codes, lists, cent, by_residual, probes=probes)
        got = be.ivfpq_search(be._f32(x[:n]), torch.from_numpy(probes), be._f32(cent) if by_residual else None, cb,
                              image, k)
        _check_backend(got, ivf_select(dis, ok, lists, probes, k), (n, qb))


@pytest.mark.parametrize("by_residual", [True, False])
def test_chunk_seam(be, oracle, by_residual):
    d, M, nlist, nprobe, k = 8, 2, 64, 64, 128
    chunk = _limits(be, M, nprobe, k)["queries_per_chunk"]
    assert chunk == (256 << 20) // (8 * nprobe * k) == 4096
    x, stored, cent, cb = _clustered(12, d, M, nlist, 400, 40)
    lists = ivf_lists(oracle, stored, cent)
    codes, _, _ = pq_encode_ref(oracle, ivfpq_encoder_input(stored, lists, cent, by_residual), cb)
    index = _index(be, cent, cb, by_residual)
    index.add_core(stored, lists)
    assert np.array_equal(_np(index.codes), codes)
    index.nprobe = nprobe
    D40, I40 = ivfpq_search_ref(oracle, x, cb, codes, lists, cent, nprobe, k, by_residual)
    assert np.all(I40[:, -1] >= 0)                                # every list probed: 400 rows for 128 places
    for n in (chunk - 1, chunk, chunk + 1):
        rep = np.arange(n) % 40                                   # 40 distinct queries repeated: every row has its reference
        got = index.search(be._f32(x[rep]), k)
        _check(got, (D40[rep], I40[rep]), n)


def test_ties_inside_a_list_and_across_two_lists(be, oracle):
    x, cb, codes, cent, inside, across = tie_codes()
    for which, by_residual in TIE_CASES:
        lists = inside if which == "inside" else across
        full = _brute_distances(x, cent, cb, codes, lists, by_residual)
        distances = ivfpq_distances(oracle, x, cb, codes, lists, cent, by_residual)
        allowed = np.ones(full.shape, bool)
        image = be.ivfpq_build(torch.from_numpy(codes), torch.from_numpy(lists), 2)
        probes, _ = be.knn(be._f32(x), be._f32(cent), 2, want_dist=False)
        cut_inside = False
        for k in (19, 20, 21, 40, 41, 128):
            ids, dist = be.ivfpq_search(be._f32(x), probes, be._f32(cent) if by_residual else None, cb, image, k)
            ref = ivfpq_search_ref(oracle, x, cb, codes, lists, cent, 2, k, by_residual, distances=distances)
            _check_backend((ids, dist), ref, (which, by_residual, k))
            cut_inside |= check_ties(_np(dist), _np(ids), full, allowed, k)
        assert cut_inside
    assert set(TIE_KS) >= {19, 20, 21, 40, 41, 128}


@pytest.mark.parametrize("by_residual", [True, False])
def test_non_finite_queries_codebooks_and_stored_rows(be, oracle, by_residual):
    d, M, nlist = 8, 2, 7
    x, stored, cent, cb = _clustered(31, d, M, nlist, 700, 30)
    x, stored = x.copy(), stored.copy()
    clean = x.copy()
    x[3, 5] = np.nan
    x[11, 0] = np.inf
    x[12, 7] = -np.inf
    x[20] = 3e38                                                  # the subtraction or the square overflows
    lists = ivf_lists(oracle, stored, cent)
    codes, _, _ = pq_encode_ref(oracle, ivfpq_encoder_input(stored, lists, cent, by_residual), cb)
    index = _index(be, cent, cb, by_residual)
    index.add(stored)
    index.nprobe = 3
    for k in (4, 128):
        ref = ivfpq_search_ref(oracle, x, cb, codes, lists, cent, 3, k, by_residual)
        assert np.all(ref[1][[3, 11, 12, 20]] == -1)
        _check(index.search(x, k), ref, ("queries", k))
        keep = [i for i in range(30) if i not in (3, 11, 12, 20)]
        cref = ivfpq_search_ref(oracle, clean, cb, codes, lists, cent, 3, k, by_residual)
        assert np.array_equal(ref[1][keep], cref[1][keep])        # the neighbours are untouched
    cbn = cb.copy()
    cbn[1, 4, 2] = np.nan                                         # a NaN word: exactly the rows using it are never listed
    pcodes = codes.copy()
    pcodes[::50, 1] = 4                                           # (an encoder never picks a NaN word: planted)
    using = np.flatnonzero(pcodes[:, 1] == 4)
    image = be.ivfpq_build(torch.from_numpy(pcodes), torch.from_numpy(lists), nlist)
    probes = ivf_probes(oracle, clean, cent, nlist)
    ref = ivfpq_search_ref(oracle, clean, cbn, pcodes, lists, cent, nlist, 128, by_residual, probes=probes)
    assert using.size >= 14 and not np.isin(ref[1], using).any()
    got = be.ivfpq_search(be._f32(clean), torch.from_numpy(probes), be._f32(cent) if by_residual else None, cbn, image, 128)
    _check_backend(got, ref, "NaN word")
    everyone = ivfpq_search_ref(oracle, clean[:2], cbn, pcodes, lists, cent, nlist, 128, by_residual, probes=probes[:2])
    assert np.all(everyone[1] >= 0)                               # ... and the other rows still are
    bad = stored.copy()                                           # non-finite stored rows
    bad[[5, 130], [2, 7]] = [np.nan, np.inf]
    blists = ivf_lists(oracle, bad, cent)
    assert blists[5] == -1 and blists[130] == -1
    fresh = _index(be, cent, cb, by_residual)
    with pytest.raises(RuntimeError, match="input contains NaN's or Inf's"):
        fresh.add(bad)
    assert fresh.ntotal == 0
    fresh.add(bad, check_finite=False)                            # counted, in no list
    assert fresh.ntotal == 700 and int(fresh.list_sizes.sum()) == 698
    bcodes, _, _ = pq_encode_ref(oracle, ivfpq_encoder_input(bad, blists, cent, by_residual), cb)
    assert np.array_equal(_np(fresh.codes), bcodes)
    forced = np.where(blists < 0, 2, blists)                      # the same rows handed to a list: codes of whatever the
    core = _index(be, cent, cb, by_residual)                      # encoder makes of them, found like any other code
    core.add_core(bad, forced)
    ccodes = _np(core.codes)
    assert int(core.list_sizes.sum()) == 700
    fresh.nprobe = core.nprobe = nlist
    for k in (4, 128):
        ref = ivfpq_search_ref(oracle, clean, cb, bcodes, blists, cent, nlist, k, by_residual)
        assert not np.isin(ref[1], [5, 130]).any()
        _check(fresh.search(clean, k), ref, ("add", k))
        _check(core.search(clean, k), ivfpq_search_ref(oracle, clean, cb, ccodes, forced, cent, nlist, k, by_residual),
               ("add_core", k))
    rec = fresh.reconstruct_n(0, 200)
    assert np.all(np.isnan(rec[[5, 130]])) and np.all(np.isfinite(np.delete(rec, [5, 130], 0)))


@pytest.mark.parametrize("ksub", [1, 7, 255])
@pytest.mark.parametrize("by_residual", [True, False])
def test_small_codebooks_and_codes_outside_them(be, oracle, ksub, by_residual):
    nlist, k = 5, 128
    for d, M in ((15, 3), (64, 8), (80, 40)):
        n = 40 if M * ksub <= 2048 else 6
        x, stored, cent, cb = _clustered(ksub + d, d, M, nlist, 300, n, ksub=ksub)
        rng = np.random.default_rng(ksub)
        lists = ivf_lists(oracle, stored, cent)
        codes = rng.integers(0, ksub, (300, M)).astype(np.uint8)
        planted = rng.choice(300, 12, replace=False)
        codes[planted, rng.integers(0, M, 12)] = rng.integers(ksub, 256, 12).astype(np.uint8)
        assert ((codes >= ksub).any(1)).sum() == 12
        image = be.ivfpq_build(torch.from_numpy(codes), torch.from_numpy(lists), nlist)
        probes = ivf_probes(oracle, x, cent, nlist)
        ref = ivfpq_search_ref(oracle, x, cb, codes, lists, cent, nlist, k, by_residual, probes=probes)
        assert not np.isin(ref[1], planted).any() and np.all(ref[1][:, :100] >= 0)
        got = be.ivfpq_search(be._f32(x), torch.from_numpy(probes), be._f32(cent) if by_residual else None, cb, image, k)
        _check_backend(got, ref, (ksub, d, M))


def test_calling_conditions_streams_and_k_prefix(be, oracle):
    d, M, nlist = 64, 8, 7
    x, stored, cent, cb = _clustered(3, d, M, nlist, 2000, 50)
    lists = ivf_lists(oracle, stored, cent)
    index = _index(be, cent, cb, True)
    index.add(stored)
    index.nprobe = 3
    codes = _np(index.codes)
    D128, I128 = ivfpq_search_ref(oracle, x, cb, codes, lists, cent, 3, 128, True)
    D, I = index.search(x, 128)                                   # host in: numpy out
    assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray)
    _check((D, I), (D128, I128), "host")
    D1, I1 = index.search(x, 1)                                   # column 0 of k = 1 is column 0 of k = 128
    assert np.array_equal(I1[:, 0], I[:, 0]) and np.array_equal(bits(D1[:, 0]), bits(D[:, 0]))
    xd, cd = be._f32(x), be._f32(cent)
    image = index._image
    probes, _ = be.knn(xd, cd, 3, want_dist=False)
    ids, none = be.ivfpq_search(xd, probes, cd, cb, image, 10, want_dist=False)
    assert none is None and np.array_equal(_np(ids), I128[:, :10])
    e_ids, e_dist = be.ivfpq_search(xd[:0], probes[:0], cd, cb, image, 5)       # n = 0
    assert tuple(e_ids.shape) == (0, 5) and tuple(e_dist.shape) == (0, 5)
    empty = be.ivfpq_build(torch.zeros((0, M), dtype=torch.uint8), torch.zeros(0, dtype=torch.int64), nlist)   # ntotal = 0
    z_ids, z_dist = be.ivfpq_search(xd, probes, cd, cb, empty, 5)
    assert np.all(_np(z_ids) == -1) and np.all(np.isposinf(_np(z_dist)))
    shifted = be.empty((x.size + 1,))                             # x offset by one float: the entry reads it by floats
    shifted[1:] = xd.reshape(-1)
    ids2, dist2 = be.ivfpq_search(shifted[1:].view(50, d), probes, cd, cb, image, 128)
    assert shifted[1:].data_ptr() % 16 == 4
    _check_backend((ids2, dist2), (D128, I128), "offset")
    torch.cuda.synchronize(be.device)
    side, other = torch.cuda.Stream(be.device), torch.cuda.Stream(be.device)
    with torch.cuda.stream(side):                                 # device in: device tensors, on the current stream
        Dd, Id = index.search(xd, 128)
    with torch.cuda.stream(other):                                # two streams at once share the context's workspace
        Do, Io = index.search(xd[:20], 33)
    with torch.cuda.stream(side):
        Dd2, Id2 = index.search(xd, 10)
    side.synchronize()
    other.synchronize()
    assert isinstance(Dd, torch.Tensor) and Dd.device == be.device and Id.device == be.device
    assert Dd.dtype == torch.float32 and Id.dtype == torch.int64
    _check((Dd, Id), (D128, I128), "side stream")
    _check((Do, Io), (D128[:20, :33], I128[:20, :33]), "other stream")
    _check((Dd2, Id2), (D128[:, :10], I128[:, :10]), "side stream again")


def test_argument_errors(be):
    AT_E_INVALID = -1
    vp = ctypes.c_void_p
    d, M, ksub, nlist, ntotal, n, k = 64, 8, 256, 3, 200, 8, 5
    rng = np.random.default_rng(1)
    cb = be._f32(rng.standard_normal((M, ksub, d // M)).astype(np.float32))
    x = be._f32(rng.standard_normal((n, d)).astype(np.float32))
    codes = torch.from_numpy(rng.integers(0, 256, (ntotal, M)).astype(np.uint8)).to(be.device)
    lists = torch.arange(ntotal, device=be.device, dtype=torch.int64) % nlist
    image = be.ivfpq_build(codes, lists, nlist)
    ngroups = image["ngroups"]
    assert ngroups == ntotal // be.IVFPQ_GROUP_ROWS + nlist
    probes = torch.arange(nlist, device=be.device, dtype=torch.int64).repeat(n, 1).contiguous()
    cent = be._f32(rng.standard_normal((nlist, d)).astype(np.float32))
    ids, dist = be.empty((n, k), torch.int64), be.empty((n, k))
    order = torch.sort(lists, stable=True).indices
    h = be.ctx.handle
    px, pp, pc, pb, pg, p2, pf, pi, pd, po, pl, pk = (vp(t.data_ptr()) for t in (
        x, probes, cent, cb, image["codes"], image["pos2id"], image["first"], ids, dist, order, lists, codes))
    search, build = be.lib.at_ivfpq_search_f32, be.lib.at_ivfpq_build
    good = (h, px, n, d, pp, nlist, nlist, pc, M, ksub, pb, pg, ngroups, p2, pf, ntotal, k, pi, pd)
    assert search(*good, None) == 0
    torch.cuda.synchronize(be.device)
    first = _np(ids).copy()
    assert np.all(first >= 0)
    assert search(*good[:18], None, None) == 0                    # no distances wanted
    a = list(good)
    a[7] = None
    assert search(*a, None) == 0                                  # no centroids: the queries as they are
    assert search(h, None, 0, d, None, nlist, nlist, None, M, ksub, None, None, ngroups, None, None, ntotal, k, None,
                  None, None) == 0                                # n == 0 touches no pointer
    torch.cuda.synchronize(be.device)

    def bad(pos, value):
        a = list(good)
        a[pos] = value
        return tuple(a)
    cases = [bad(0, None), bad(2, -1), bad(3, 0), bad(3, 63), bad(5, 0), bad(5, -1), bad(5, (1 << 24) + 1), bad(6, 0),
             bad(6, (1 << 24) + 1), bad(8, 0), bad(8, 65), bad(9, 0), bad(9, 257), bad(12, 0), bad(12, 1 << 27),
             bad(15, -1), bad(15, 1 << 31), bad(16, 0), bad(16, 129), bad(1, None), bad(4, None), bad(10, None),
             bad(11, None), bad(13, None), bad(14, None), bad(17, None)]
    ids.fill_(7)
    for a in cases:
        assert search(*a, None) == AT_E_INVALID, a
        assert b"at_ivfpq_search_f32" in be.lib.at_last_error()
    torch.cuda.synchronize(be.device)
    assert bool((ids == 7).all())                                 # nothing was launched
    gb = (h, pk, pl, po, ntotal, M, nlist, ngroups, pg, p2, pf)
    assert build(*gb, None) == 0

    def badb(pos, value):
        a = list(gb)
        a[pos] = value
        return tuple(a)
    for a in [badb(0, None), badb(4, -1), badb(4, 1 << 31), badb(5, 0), badb(5, 65), badb(6, 0), badb(6, (1 << 24) + 1),
              badb(7, ngroups - 1), badb(7, 1 << 27), badb(1, None), badb(2, None), badb(3, None), badb(8, None),
              badb(9, None), badb(10, None)]:
        assert build(*a, None) == AT_E_INVALID, a
        assert b"at_ivfpq_build" in be.lib.at_last_error()
    torch.cuda.synchronize(be.device)
    assert search(*good, None) == 0                               # the image is as it was
    torch.cuda.synchronize(be.device)
    assert np.array_equal(_np(ids), first)
    lim = be.lib.at_ivfpq_search_limits
    for args in ((0, 1, 1), (65, 1, 1), (8, 0, 1), (8, 1, 0), (8, 1, 129)):
        assert lim(None, None, None, *args) == AT_E_INVALID and b"at_ivfpq_search_limits" in be.lib.at_last_error()
    assert be.ivfpq_search_limits(32, 1, 1)["pairs_per_block"] == 4 and be.ivfpq_search_limits(33, 1, 1)["pairs_per_block"] == 2
    with pytest.raises(RuntimeError, match="at least 1"):
        be.ivfpq_search(x, probes, cent, cb, image, 0)
    with pytest.raises(ValueError):
        be.ivfpq_search(x, probes, cent, cb[:4], image, 3)


def test_end_to_end_on_the_device(be, oracle):
    from audio_tokens_amd.ops import IndexFlatL2, IndexIVFPQ
    d, M, nlist = 64, 8, 16
    rng = np.random.default_rng(8)
    centres = rng.standard_normal((40, d)).astype(np.float32)
    x = (centres[rng.integers(0, 40, 6000)] + 0.5 * rng.standard_normal((6000, d))).astype(np.float32)
    q = x[:30] + 0.05 * rng.standard_normal((30, d)).astype(np.float32)
    index = IndexIVFPQ(IndexFlatL2(d, backend=be), d, nlist, M, niter=3, backend=be)
    assert not index.is_trained
    index.train(x)
    assert index.is_trained and index.quantizer.ntotal == nlist and index.pq.centroids.shape == (M, 256, d // M)
    index.add(x[:2500])
    index.add(be._f32(x[2500:]))
    assert index.ntotal == 6000 and int(index.list_sizes.sum()) == 6000
    cent, cb, codes = _np(index.quantizer._c), index.pq.centroids, _np(index.codes)
    lists = ivf_lists(oracle, x, cent)
    want, _, _ = pq_encode_ref(oracle, ivfpq_encoder_input(x, lists, cent, True), cb)
    assert np.array_equal(codes, want) and np.array_equal(index.list_sizes, np.bincount(lists, minlength=nlist))
    index.nprobe = 4
    ref = ivfpq_search_ref(oracle, q, cb, codes, lists, cent, 4, 10, True)
    D, I = index.search(q, 10)
    assert isinstance(D, np.ndarray)
    _check((D, I), ref, "host input")
    Dd, Id = index.search(be._f32(q), 10)
    assert isinstance(Dd, torch.Tensor) and Dd.device == be.device
    _check((Dd, Id), ref, "device input")
    rec = index.reconstruct_n(100, 50)
    assert np.array_equal(bits(rec), bits(pq_decode_ref(codes[100:150], cb) + cent[lists[100:150]]))
    assert np.array_equal(bits(index.reconstruct(7)), bits(pq_decode_ref(codes[7:8], cb)[0] + cent[lists[7]]))
    index.reset()
    assert index.ntotal == 0 and index.is_trained and np.all(_np(index.search(q, 3)[1]) == -1)
    index.add(x[3000:4000])
    ref2 = ivfpq_search_ref(oracle, q, cb, codes[3000:4000], lists[3000:4000], cent, 4, 10, True)
    _check(index.search(q, 10), ref2, "after reset")
