"""The quantisers and the inner-product routes on the hard data of tests/hard_quantiser_data.py, on the MI355X, bit for
bit against the CPU references (pq_ref, rq_ref, rq_beam_ref, pq_search_ref, spherical_ref): every row of every rung,
nothing exempt.  tests/test_hard_quantiser_ref.py proves that the rungs are what their names say."""
import functools
import warnings

import numpy as np
import pytest
import torch

import hard_quantiser_data as hq
from knn_ref import select
from pq_ref import pq_encode_ref
from pq_search_ref import pq_distances, pq_tables
from rq_beam_ref import rq_beam_encode_ref, rq_beam_step_ref
from rq_ref import rq_decode_ref, rq_encode_ref
from spherical_ref import renorm_ref, search_ip_ref, spherical_kmeans_ref

pytestmark = pytest.mark.gpu

PQ_NAMES = ("big", "small", "sub", "fade", "zero", "unlisted")
# (d, M): the <8> and <4> register instances, <16>, and the run-time dsub instance (dsub = 24)
PQ_SHAPES = [(64, 8), (64, 16), (128, 8), (96, 4)]
RQ_NAMES = hq.SCALED_NAMES + ("unlisted",) + hq.OFF_NAMES
RQ_SHAPES = [(64, 4), (128, 4), (12, 3)]        # rq_fused_kernel<1>, <2>; the general kernel
BEAM_NAMES = ("big", "sub", "fade", "zero", "unlisted", "clamp", "flat")
BEAM_ROWS = {5: hq.N, 32: 289}                  # B = 32: 9 tiles + one row, 9248 beam rows behind stage 0
SEARCH_NAMES = ("big", "sub", "zero", "unlisted")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _off_by_one_float(be, a):
    """The rows of a on the device, contiguous, 4 bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.zeros(a.size + 4, device=be.device)
    view = buf[1:1 + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _same(got, ref, names, label):
    """Every array of got (device) has the bytes of its reference; then the flag."""
    for name, g, r in zip(names, got, ref):
        g = _np(g)
        assert g.dtype == r.dtype and g.shape == r.shape, (label, name, g.dtype, g.shape, r.dtype, r.shape)
        wrong = np.argwhere(g.reshape(g.shape[0], -1).view(np.uint8) != r.reshape(r.shape[0], -1).view(np.uint8))
        assert wrong.size == 0, (label, name, len(wrong), wrong[:4], g[wrong[0][0]], r[wrong[0][0]])
    assert int(got[len(names)].item()) == int(ref[len(names)]), (label, "flag")


@functools.lru_cache(maxsize=None)
def _pq_ref(oracle, name, d, M, rows=None, clean=False):
    r = hq.pq_rung(oracle, name, d, M)
    x = r["x_clean"] if clean else r["x"]
    return pq_encode_ref(oracle, x if rows is None else x[:rows], r["cb"])


@functools.lru_cache(maxsize=None)
def _rq_ref(oracle, name, d, M, ksub=256, rows=None, clean=False):
    r = hq.rq_rung(oracle, name, d, M, ksub)
    x = r["x_clean"] if clean else r["x"]
    return rq_encode_ref(oracle, x if rows is None else x[:rows], r["cb"])


def _planted(r, n):
    keep = np.ones(n, bool)
    keep[r["overflow"]] = False
    keep[r["edge_sum"]] = False
    return keep


# ---------------------------------------------------------------------------------------------------------------------
# be.pq_encode

@pytest.mark.parametrize("d,M", PQ_SHAPES)
@pytest.mark.parametrize("name", PQ_NAMES)
def test_pq_encode(be, oracle, name, d, M):
    r = hq.pq_rung(oracle, name, d, M)
    x, cbd = r["x"], be._f32(r["cb"])
    names = ("codes", "dist")
    ref = _pq_ref(oracle, name, d, M)
    got = be.pq_encode(x, cbd, want_dist=True)
    _same(got, ref, names, (name, d, M))
    codes, none, bad = be.pq_encode(x, cbd)
    assert none is None and np.array_equal(_np(codes), ref[0]) and int(bad.item()) == int(ref[2])
    # the general path: the direct form (fewer than 20 rows), and rows off a 16-byte boundary
    _same(be.pq_encode(x[:19], cbd, want_dist=True), _pq_ref(oracle, name, d, M, rows=19), names, (name, d, M, 19))
    _same(be.pq_encode(_off_by_one_float(be, x), cbd, want_dist=True), ref, names, (name, d, M, "offset"))
    if name == "unlisted":                        # the neighbours of the planted rows: as without them
        keep = _planted(r, hq.N)
        clean = be.pq_encode(r["x_clean"], cbd, want_dist=True)
        _same(clean, _pq_ref(oracle, name, d, M, clean=True), names, (name, d, M, "clean"))
        assert np.array_equal(_np(got[0])[keep], _np(clean[0])[keep])
        assert np.array_equal(bits(_np(got[1])[keep]), bits(_np(clean[1])[keep]))
        assert int(got[2].item()) == 1


# ---------------------------------------------------------------------------------------------------------------------
# be.rq_encode / be.rq_decode

RQ_OUT = ("codes", "dist", "residual")


@pytest.mark.parametrize("d,M", RQ_SHAPES)
@pytest.mark.parametrize("name", RQ_NAMES)
def test_rq_encode(be, oracle, name, d, M):
    r = hq.rq_rung(oracle, name, d, M)
    x, cbd = r["x"], be._f32(r["cb"])
    ref = _rq_ref(oracle, name, d, M)
    got = be.rq_encode(x, cbd, want_dist=True, want_residual=True)
    _same(got, ref, RQ_OUT, (name, d, M))
    # the general kernel: fewer than 20 rows (the direct form), and rows off a 16-byte boundary
    _same(be.rq_encode(x[:19], cbd, want_dist=True, want_residual=True), _rq_ref(oracle, name, d, M, rows=19), RQ_OUT,
          (name, d, M, 19))
    _same(be.rq_encode(_off_by_one_float(be, x), cbd, want_dist=True, want_residual=True), ref, RQ_OUT, (name, d, M, "offset"))
    codes, none, none2, bad = be.rq_encode(x, cbd)
    assert none is None and none2 is None and np.array_equal(_np(codes), ref[0]) and int(bad.item()) == int(ref[3])
    if name == "unlisted":
        keep = _planted(r, hq.N)
        clean = be.rq_encode(r["x_clean"], cbd, want_dist=True, want_residual=True)
        _same(clean, _rq_ref(oracle, name, d, M, clean=True), RQ_OUT, (name, d, M, "clean"))
        for j in range(3):
            assert np.array_equal(_np(got[j])[keep].view(np.uint8), _np(clean[j])[keep].view(np.uint8)), j
        assert int(got[3].item()) == 1 and int(clean[3].item()) == 0


@pytest.mark.parametrize("d,M", RQ_SHAPES)
def test_rq_encode_fade_with_a_second_tile_of_one_word(be, oracle, d, M):
    r = hq.rq_rung(oracle, "fade", d, M, 129)
    _same(be.rq_encode(r["x"], r["cb"], want_dist=True, want_residual=True), _rq_ref(oracle, "fade", d, M, 129), RQ_OUT,
          (d, M, 129))


@pytest.mark.parametrize("d,M", RQ_SHAPES)
@pytest.mark.parametrize("name", ["big", "sub", "zero"])
def test_rq_decode(be, oracle, name, d, M):
    r = hq.rq_rung(oracle, name, d, M)
    codes = _rq_ref(oracle, name, d, M)[0]
    with np.errstate(all="ignore"):
        want = rq_decode_ref(codes, r["cb"])
    assert np.array_equal(bits(_np(be.rq_decode(codes, r["cb"]))), bits(want))


# ---------------------------------------------------------------------------------------------------------------------
# be.rq_beam_encode / be.rq_beam_step

@pytest.mark.parametrize("d,M", [(64, 3), (12, 3)])
@pytest.mark.parametrize("B", [5, 32])
@pytest.mark.parametrize("name", BEAM_NAMES)
def test_rq_beam_encode(be, oracle, name, B, d, M):
    n = BEAM_ROWS[B]
    r = hq.rq_rung(oracle, name, d, M, n=n)
    cbd = be._f32(r["cb"])
    ref = rq_beam_encode_ref(oracle, r["x"], r["cb"], B)
    got = be.rq_beam_encode(r["x"], cbd, B, want_dist=True, want_residual=True)
    _same(got, ref, RQ_OUT, (name, B, d, M))
    if name == "unlisted":
        keep = _planted(r, n)
        clean = be.rq_beam_encode(r["x_clean"], cbd, B, want_dist=True, want_residual=True)
        for j in range(3):
            assert np.array_equal(_np(got[j])[keep].view(np.uint8), _np(clean[j])[keep].view(np.uint8)), j
        assert int(got[3].item()) == 1 and int(clean[3].item()) == 0


@pytest.mark.parametrize("d", [64, 12])
@pytest.mark.parametrize("name", ["zero", "flat"])
def test_rq_beam_step_when_everything_ties(be, oracle, name, d):
    """b_in = 5 beams, b_out = 32 slots, every candidate of stage 0 at +0 (zero: of stage 1 as well): the order is
    (parent slot, word) alone.  Parent, code, distance and the residual of every slot."""
    r = hq.rq_rung(oracle, name, d, 3)
    first = rq_beam_step_ref(oracle, r["x"].reshape(hq.N, 1, d), 1, r["cb"][0], 5)
    assert np.all(bits(first[3]) == 0)
    ref = rq_beam_step_ref(oracle, first[0], 5, r["cb"][1], 32)
    if name == "zero":
        assert np.all(bits(ref[3]) == 0) and np.all(ref[1] == 0)
    out = ("r_out", "parent", "code", "dist")
    got1 = be.rq_beam_step(r["x"], 1, r["cb"][0], 5)
    _same(got1, first, out, (name, d, "stage 0"))
    _same(be.rq_beam_step(first[0], 5, r["cb"][1], 32), ref, out, (name, d, "stage 1"))
    _same(be.rq_beam_step(r["x"], 1, r["cb"][0], 32), rq_beam_step_ref(oracle, r["x"].reshape(hq.N, 1, d), 1, r["cb"][0], 32),
          out, (name, d, "stage 0, 32 slots"))


# ---------------------------------------------------------------------------------------------------------------------
# be.pq_search / ops.IndexPQ

@functools.lru_cache(maxsize=None)
def _search_ref(oracle, name, d, M):
    cs = hq.pq_search_case(oracle, name, d, M)
    with np.errstate(all="ignore"):
        T = pq_tables(oracle, cs["x"], cs["cb"])
        dis, ok = pq_distances(T, cs["codes"])
    return {k: select(dis, ok, k) for k in (1, 10, 128)}


@pytest.mark.parametrize("d,M", [(64, 8), (128, 64)])   # four and two queries per workgroup
@pytest.mark.parametrize("name", SEARCH_NAMES)
def test_pq_search(be, oracle, name, d, M):
    cs = hq.pq_search_case(oracle, name, d, M)
    lim = be.pq_search_limits(M, hq.NTOTAL, 128)
    assert lim["slab_rows"] == hq.SLAB and lim["queries_per_block"] == (4 if M == 8 else 2)
    cbd, xd, cd = be._f32(cs["cb"]), be._f32(cs["x"]), be.from_host(cs["codes"])
    for k, (D, I) in _search_ref(oracle, name, d, M).items():
        ids, dist = be.pq_search(xd, cbd, cd, k)
        ids, dist = _np(ids), _np(dist)
        wrong = np.argwhere((ids != I) | (bits(dist) != bits(D)))
        assert wrong.size == 0, (name, d, M, k, len(wrong), wrong[:4], ids[tuple(wrong[0])], I[tuple(wrong[0])],
                                 dist[tuple(wrong[0])], D[tuple(wrong[0])])
    if name == "unlisted":                        # the ordinary queries: as in a call of their own
        plain = np.arange(8, 24)
        ids, dist = be.pq_search(xd[8:], cbd, cd, 128)
        D, I = _search_ref(oracle, name, d, M)[128]
        assert np.array_equal(_np(ids), I[plain]) and np.array_equal(bits(_np(dist)), bits(D[plain]))


def test_index_pq_on_sub(be, oracle):
    from audio_tokens_amd.ops import IndexPQ
    cs = hq.pq_search_case(oracle, "sub", 64, 8)
    index = IndexPQ(64, 8, backend=be)
    index.pq.set_centroids(cs["cb"])
    index.add_codes(cs["codes"][:40000])
    index.add_codes(be.from_host(cs["codes"][40000:]))
    assert index.ntotal == hq.NTOTAL
    D, I = index.search(cs["x"], 10)
    Dr, Ir = _search_ref(oracle, "sub", 64, 8)[10]
    assert isinstance(D, np.ndarray) and np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))
    assert np.all(D < np.float32(2.0 ** -126)) and np.array_equal(I[:, 0], np.arange(24))


# ---------------------------------------------------------------------------------------------------------------------
# the inner-product routes

@functools.lru_cache(maxsize=None)
def _ip_ref(oracle, name, d):
    r = hq.ip_rung(oracle, name, d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return search_ip_ref(r["x"], r["c"])


@pytest.mark.parametrize("d", [64, 128, 200, 6])         # register-resident; multi-chunk, partial last chunk; scalar
@pytest.mark.parametrize("name", hq.IP_NAMES)
def test_assign_ip(be, oracle, name, d):
    r = hq.ip_rung(oracle, name, d)
    ids_r, ip_r = _ip_ref(oracle, name, d)
    ids, ip = be.assign_ip(be.from_host(r["x"]), be.from_host(r["c"]))
    ids, ip = _np(ids), _np(ip)
    wrong = np.flatnonzero((ids != ids_r) | (bits(ip) != bits(ip_r)))
    assert wrong.size == 0, (name, d, len(wrong), wrong[:5], ids[wrong[:5]], ids_r[wrong[:5]], ip[wrong[:5]], ip_r[wrong[:5]])
    ids2, none = be.assign_ip(_off_by_one_float(be, r["x"]), be.from_host(r["c"]), want_dist=False)
    assert none is None and np.array_equal(_np(ids2), ids_r)


@pytest.mark.parametrize("name", ["ipinf", "zero"])
def test_index_flat_ip_search(be, oracle, name):
    from audio_tokens_amd.ops import IndexFlatIP
    r = hq.ip_rung(oracle, name, 64)
    ids_r, ip_r = _ip_ref(oracle, name, 64)
    index = IndexFlatIP(64, backend=be)
    index.add(r["c"])
    D, I = index.search(r["x"], 1)
    assert np.array_equal(I[:, 0], ids_r) and np.array_equal(bits(D[:, 0]), bits(ip_r))


@pytest.mark.parametrize("d", [64, 6, 200])
def test_renorm_rows(be, d):
    c = hq.renorm_rows_case(d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = renorm_ref(c)
    t = be.from_host(c)
    be.renorm_rows(t)
    assert np.array_equal(bits(_np(t)), bits(ref))


@pytest.mark.parametrize("e", [50, -40])
def test_spherical_kmeans_far_from_unit_scale(be, oracle, e):
    from audio_tokens_amd.ops import Kmeans
    x = hq.spherical_rows(oracle, e)
    km = Kmeans(64, 64, niter=4, spherical=True, backend=be)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km.train(x)
        r = spherical_kmeans_ref(x, 64, 4)
        ids_r, ip_r = search_ip_ref(x, r.centroids)
    assert np.array_equal(bits(km.centroids), bits(r.centroids))
    assert [s["nsplit"] for s in km.iteration_stats] == r.nsplit
    ids, ip = be.assign_ip(be.from_host(x), km.centroids_device)
    assert np.array_equal(_np(ids), ids_r) and np.array_equal(bits(_np(ip)), bits(ip_r))
