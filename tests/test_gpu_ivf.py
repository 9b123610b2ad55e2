"""ops.IndexIVFFlat / HipBackend.ivf_build / ivf_search / at_ivf_*_f32 on the MI355X, ids and distance bits against
tests/ivf_ref.py (the oracle's expansion-form distances, knn_ref's probes and selection) on every row of every case.
The shapes are the smallest at which every path of csrc/ivf.hip runs: d = 64 / 128 (queries in registers), 40 (re-read
form), 39 (queries padded to 40); lists of 0, 1, 128 and 129 rows (a tile is 128 rows); 257 queries, so that a list
probed by all of them takes three blocks of 128; every list-width class of the per-lane top-k (k = 1, 4, 10, 32)."""
import ctypes

import numpy as np
import pytest
import torch

from ivf_ref import check_ties, ivf_distances, ivf_lists, ivf_probes, ivf_search_ref, ivf_select, tie_case

pytestmark = pytest.mark.gpu

NTOTAL, NQ = 3000, 257
NS, KS = (1, 19, 20, 257), (1, 4, 10, 32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def _check(got, ref, label=""):
    """got: (D, I) of IndexIVFFlat.search; ref: (D, I) of the reference."""
    dist, ids = _np(got[0]), _np(got[1])
    D, I = ref
    assert ids.dtype == np.int64 and dist.dtype == np.float32 and ids.shape == I.shape and dist.shape == D.shape, label
    wrong = np.argwhere((ids != I) | (bits(dist) != bits(D)))
    assert wrong.size == 0, (label, len(wrong), wrong[:5], ids[tuple(wrong[0])], I[tuple(wrong[0])],
                             dist[tuple(wrong[0])], D[tuple(wrong[0])])


def _clustered(seed, d, nlist, ntotal=NTOTAL, nq=NQ):
    """nlist centres, stored rows and queries scattered round them (so lists and probes mean something)."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    stored = (cent[rng.integers(0, nlist, ntotal)] + 0.7 * rng.standard_normal((ntotal, d))).astype(np.float32)
    x = (cent[rng.integers(0, nlist, nq)] + 0.7 * rng.standard_normal((nq, d))).astype(np.float32)
    return x, stored, cent


def _index(be, cent, nlist=None):
    from audio_tokens_amd.ops import IndexFlatL2, IndexIVFFlat
    quant = IndexFlatL2(cent.shape[1], backend=be)
    if cent.shape[0]:
        quant.add(cent)
    return IndexIVFFlat(quant, cent.shape[1], nlist or cent.shape[0], backend=be)


_CASES = {}


def _case(oracle, d, nlist):
    """Data and reference of one (d, nlist), computed once and left unchanged."""
    if (d, nlist) not in _CASES:
        x, stored, cent = _clustered(100 * d + nlist, d, nlist)
        lists = ivf_lists(oracle, stored, cent)
        _CASES[(d, nlist)] = (x, stored, cent, lists, ivf_distances(oracle, x, stored))
    return _CASES[(d, nlist)]


@pytest.mark.parametrize("nlist", [7, 61])
@pytest.mark.parametrize("d", [64, 128, 40, 39])
def test_grid_bit_exact(be, oracle, d, nlist):
    x, stored, cent, lists, (dis, ok) = _case(oracle, d, nlist)
    assert np.all(lists >= 0)
    index = _index(be, cent)
    index.add(stored)
    assert index.ntotal == NTOTAL and np.array_equal(index.list_sizes, np.bincount(lists, minlength=nlist))
    for n in NS:
        for nprobe in (1, 3, nlist, nlist + 5):
            probes = ivf_probes(oracle, x[:n], cent, nprobe)     # (n < 20: the direct form decides the probes)
            if n == NQ and nprobe >= nlist:                       # every list is probed by 257 queries: three blocks
                assert all(np.count_nonzero(probes == l) == NQ for l in range(nlist))
            index.nprobe = nprobe
            for k in KS:
                ref = ivf_select(dis[:n], ok[:n], lists, probes, k)
                _check(index.search(x[:n], k), ref, (d, nlist, n, nprobe, k))


@pytest.mark.parametrize("d,nlist", [(64, 7), (40, 61)])
def test_equals_the_flat_search_when_every_list_is_probed(be, oracle, d, nlist):
    from audio_tokens_amd.ops import IndexFlatL2
    x, stored, cent, lists, _ = _case(oracle, d, nlist)
    assert np.all(lists >= 0)                                     # no stored row is unlisted
    index = _index(be, cent)
    index.add(stored)
    index.nprobe = nlist
    flat = IndexFlatL2(d, backend=be)
    flat.add(stored)
    xd = be._f32(x)
    for n in (20, NQ):
        for k in KS:
            (D, I), (Df, If) = index.search(xd[:n], k), flat.search(xd[:n], k)
            assert torch.equal(I, If) and torch.equal(D.view(torch.int32), Df.view(torch.int32)), (n, k)


def test_constructed_lists_and_under_full_results(be, oracle):
    d, nlist, k = 64, 7, 10
    rng = np.random.default_rng(77)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    cent[4] += 40.0                                               # far from every query: nobody probes list 4
    sizes = [0, 1, 128, 129, 300, 500, 942]
    given = np.concatenate([np.full(s, l, np.int64) for l, s in enumerate(sizes)])
    given = given[rng.permutation(given.size)]
    stored = rng.standard_normal((given.size, d)).astype(np.float32)   # (the lists are the caller's: rows lie anywhere)
    x = (cent[rng.integers(0, 4, 60)] + 0.3 * rng.standard_normal((60, d))).astype(np.float32)
    # the preconditions, on the test's own data
    assert np.array_equal(np.bincount(given, minlength=nlist), sizes)
    assert sizes[0] == 0 and sizes[1] == 1 and sizes[2] == be.IVF_TILE_ROWS and sizes[3] == be.IVF_TILE_ROWS + 1
    index = _index(be, cent)
    index.add_core(stored, given)
    assert np.array_equal(index.list_sizes, sizes)
    distances = ivf_distances(oracle, x, stored)
    for nprobe in (1, 3):
        probes = ivf_probes(oracle, x, cent, nprobe)
        assert not np.any(probes == 4) and all(np.any(probes == l) for l in (0, 1, 2, 3))
        index.nprobe = nprobe
        D, I = ivf_select(*distances, given, probes, k)
        _check(index.search(x, k), (D, I), nprobe)
        if nprobe == 1:                                           # queries of lists 0 and 1 find fewer than k rows
            short = I[:, -1] == -1
            assert 0 < np.count_nonzero(short) < x.shape[0]
            assert np.any(np.all(I == -1, 1)) and np.any(short & (I[:, 0] >= 0))
            assert np.all(np.isposinf(D[I == -1])) and np.all(np.isfinite(D[I >= 0]))


def test_non_finite_queries_and_stored_rows(be, oracle):
    d, nlist = 64, 7
    x, stored, cent, _, _ = _case(oracle, d, nlist)
    x, stored = x[:40].copy(), stored[:700].copy()
    x[3, 9] = np.nan
    x[11, 0] = np.inf
    stored[[5, 130], [2, 63]] = np.nan
    stored[300] = 3e19                                            # |r|^2 overflows
    lists = ivf_lists(oracle, stored, cent)
    assert lists[5] == -1 and lists[130] == -1 and lists[300] == -1 and np.count_nonzero(lists < 0) == 3
    distances = ivf_distances(oracle, x, stored)
    index = _index(be, cent)
    with pytest.raises(RuntimeError, match="input contains NaN's or Inf's"):
        index.add(stored)
    assert index.ntotal == 0
    index.add(stored, check_finite=False)                         # counted, in no list
    assert index.ntotal == 700 and int(index.list_sizes.sum()) == 697
    forced = np.where(lists < 0, 2, lists)                        # the same rows handed to a list: still never listed
    core = _index(be, cent)
    core.add_core(stored, forced)
    assert int(core.list_sizes.sum()) == 700
    for nprobe in (2, nlist):
        index.nprobe = core.nprobe = nprobe
        for k in (4, 32):
            ref = ivf_search_ref(oracle, x, stored, lists, cent, nprobe, k, distances=distances)
            assert np.all(ref[1][[3, 11]] == -1) and not np.isin(ref[1], [5, 130, 300]).any()
            _check(index.search(x, k), ref, ("add", nprobe, k))
            _check(core.search(x, k), ivf_search_ref(oracle, x, stored, forced, cent, nprobe, k, distances=distances),
                   ("add_core", nprobe, k))
            assert not np.isin(core.search(x, k)[1], [5, 130, 300]).any()


def test_ties_inside_a_list_and_across_two_lists(be, oracle):
    x, stored, inside, across = tie_case()
    cent = np.zeros((2, 8), np.float32)
    cent[1, 0] = 0.125                                            # two lists, both probed with nprobe = 2
    full = ((x.astype(np.float64)[:, None, :] - stored.astype(np.float64)[None, :, :]) ** 2).sum(2)
    distances = ivf_distances(oracle, x, stored)
    allowed = np.ones(full.shape, bool)
    cut_inside = False
    for lists in (inside, across):
        index = _index(be, cent)
        index.add_core(stored, lists)
        index.nprobe = 2
        for k in (1, 19, 20, 21, 32):
            D, I = index.search(x, k)
            _check((D, I), ivf_search_ref(oracle, x, stored, lists, cent, 2, k, distances=distances), k)
            cut_inside |= check_ties(D, I, full, allowed, k)
    assert cut_inside


def test_trained_quantiser_and_tokens_as_list_numbers(be, oracle):
    from audio_tokens_amd.ops import IndexFlatL2, IndexIVFFlat
    d, nlist = 64, 7
    x, stored, _, _, _ = _case(oracle, d, nlist)
    trained = IndexIVFFlat(IndexFlatL2(d, backend=be), d, nlist, backend=be)
    assert not trained.is_trained
    trained.train(stored)
    assert trained.is_trained and trained.quantizer.ntotal == nlist
    trained.add(stored)
    vocabulary = IndexFlatL2(d, backend=be)                       # the pipeline's way: centroids in, tokens out
    vocabulary.add(trained.quantizer._c)
    tokens, _ = vocabulary.assign(be._f32(stored))
    ready = IndexIVFFlat(vocabulary, d, nlist, backend=be)
    assert ready.is_trained
    ready.add_core(stored, tokens)
    assert np.array_equal(ready.list_sizes, trained.list_sizes) and int(ready.list_sizes.sum()) == NTOTAL
    cent = _np(trained.quantizer._c)
    lists = ivf_lists(oracle, stored, cent)
    for nprobe in (1, 3):
        trained.nprobe = ready.nprobe = nprobe
        (Da, Ia), (Db, Ib) = trained.search(x, 10), ready.search(x, 10)
        assert np.array_equal(Ia, Ib) and np.array_equal(bits(Da), bits(Db))
        _check((Da, Ia), ivf_search_ref(oracle, x, stored, lists, cent, nprobe, 10), nprobe)


def test_streams_return_types_and_incremental_adds(be, oracle):
    d, nlist = 128, 7
    x, stored, cent, lists, distances = _case(oracle, d, nlist)
    ref = ivf_search_ref(oracle, x, stored, lists, cent, 3, 10, distances=distances)
    whole, parts = _index(be, cent), _index(be, cent)
    whole.add(stored)
    parts.add(stored[:1700])
    between = parts.search(x[:30], 2)                             # a search between the adds: the image is rebuilt
    assert np.all(between[1] < 1700)
    parts.add(be._f32(stored[1700:]))
    whole.nprobe = parts.nprobe = 3
    D, I = whole.search(x, 10)                                    # host in: numpy out
    assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray)
    _check((D, I), ref, "host")
    _check(parts.search(x, 10), ref, "two adds")
    xd = be._f32(x)
    torch.cuda.synchronize(be.device)
    side = torch.cuda.Stream(be.device)
    with torch.cuda.stream(side):                                 # device in: device tensors, on the current stream
        fresh = _index(be, cent)
        fresh.add(be._f32(stored))
        fresh.nprobe = 3
        Dd, Id = fresh.search(xd, 10)
    side.synchronize()
    assert isinstance(Dd, torch.Tensor) and Dd.device == be.device and Id.device == be.device
    assert Dd.dtype == torch.float32 and Id.dtype == torch.int64
    _check((Dd, Id), ref, "side stream")


def test_argument_errors_and_empty_calls(be):
    AT_E_INVALID = -1
    vp = ctypes.c_void_p
    d, nlist, ntotal, n, k = 64, 3, 200, 8, 5
    rows = be._f32(np.random.default_rng(1).standard_normal((ntotal, d)).astype(np.float32))
    lists = torch.arange(ntotal, device=be.device, dtype=torch.int64) % nlist
    image = be.ivf_build(rows, lists, nlist)
    ntiles = image["ntiles"]
    assert ntiles == ntotal // be.IVF_TILE_ROWS + nlist
    x = rows[:n].contiguous()
    probes = torch.arange(nlist, device=be.device, dtype=torch.int64).repeat(n, 1).contiguous()
    ids, dist = be.empty((n, k), torch.int64), be.empty((n, k))
    order = torch.sort(lists, stable=True).indices
    h = be.ctx.handle
    px, pp, pg, p2, pf, pi, pd, pr, pl, po = (vp(t.data_ptr()) for t in (x, probes, image["img"], image["pos2id"],
                                                                         image["first"], ids, dist, rows, lists, order))
    search, build = be.lib.at_ivf_search_f32, be.lib.at_ivf_build_f32
    good = (h, px, n, d, pp, nlist, nlist, pg, ntiles, p2, pf, ntotal, k, pi, pd)
    assert search(*good, None) == 0
    assert search(*good[:14], None, None) == 0                    # no distances wanted
    torch.cuda.synchronize(be.device)
    got = _np(ids)
    assert got[:, 0].tolist() == list(range(n)) and bool((dist[:, 0] == 0).all())   # every query is a stored row
    assert search(h, None, 0, d, None, nlist, nlist, None, ntiles, None, None, ntotal, k, None, None, None) == 0   # n == 0

    def bad(pos, value):
        a = list(good)
        a[pos] = value
        return tuple(a)
    cases = [bad(0, None), bad(2, -1), bad(3, 0), bad(3, 62), bad(5, 0), bad(5, -1), bad(6, 0), bad(8, 0), bad(11, -1),
             bad(11, 1 << 31), bad(12, 0), bad(12, 33), bad(1, None), bad(4, None), bad(7, None), bad(9, None),
             bad(10, None), bad(13, None), bad(1, vp(x.data_ptr() + 4))]
    ids.fill_(7)
    for a in cases:
        assert search(*a, None) == AT_E_INVALID, a
        assert b"at_ivf_search_f32" in be.lib.at_last_error()
    torch.cuda.synchronize(be.device)
    assert bool((ids == 7).all())                                 # nothing was launched
    gb = (h, pr, pl, po, ntotal, d, nlist, ntiles, pg, p2, pf)
    assert build(*gb, None) == 0

    def badb(pos, value):
        a = list(gb)
        a[pos] = value
        return tuple(a)
    for a in [badb(0, None), badb(4, -1), badb(4, 1 << 31), badb(5, 0), badb(6, 0), badb(7, ntiles - 1), badb(1, None),
              badb(2, None), badb(3, None), badb(8, None), badb(9, None), badb(10, None)]:
        assert build(*a, None) == AT_E_INVALID, a
        assert b"at_ivf_build_f32" in be.lib.at_last_error()
    torch.cuda.synchronize(be.device)
    assert search(*good, None) == 0                               # the image is as it was
    torch.cuda.synchronize(be.device)
    assert _np(ids)[:, 0].tolist() == list(range(n))
    with pytest.raises(RuntimeError, match="at least 1"):
        be.ivf_search(x, probes, image, 0)
