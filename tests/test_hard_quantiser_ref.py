"""The rungs of tests/hard_quantiser_data.py are what their names say: proved with the CPU references alone (pq_ref,
rq_ref, rq_beam_ref, pq_search_ref, spherical_ref, knn_ref).  tests/test_gpu_hard_quantisers.py compares the kernels with
the same references bit for bit; without the facts below a rung that silently degenerated would make that vacuous."""
import warnings

import numpy as np
import pytest

import hard_quantiser_data as hq
import magnitude_data as md
from knn_ref import select
from pq_ref import pq_encode_ref
from pq_search_ref import pq_distances, pq_tables
from rq_beam_ref import rq_beam_encode_ref, rq_beam_step_ref
from rq_ref import rq_encode_ref
from spherical_ref import ip_matrix, renorm_ref, search_ip_ref, spherical_kmeans_ref

FUSED = [(64, 4), (128, 4)]
TINY = np.float32(2.0 ** -126)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _enc(oracle, name, d, M, **kw):
    r = hq.rq_rung(oracle, name, d, M, **kw)
    return r, rq_encode_ref(oracle, r["x"], r["cb"])


@pytest.mark.parametrize("d,M", FUSED + [(12, 3)])
def test_the_control_and_the_big_exponent(oracle, d, M):
    x, cb, pick = hq.rq_table(oracle, 9, hq.N, d, M)
    assert x.shape == (hq.N, d) and hq.N == 33 * 32 + 1
    for m in range(M):
        nrm = np.sqrt((cb[m].astype(np.float64) ** 2).sum(1)) * 2.0 ** m
        assert np.abs(nrm - 1).max() < 1e-6                                   # unit words x 2^-m
        assert np.array_equal(cb[m][128:148], cb[m][0:20])
    on = sum(cb[m][pick[:hq.ON_SUM, m]] for m in range(M))
    assert np.array_equal(bits(x[:hq.ON_SUM]), bits(on))
    codes, dist, res, bad = rq_encode_ref(oracle, x, cb)
    assert not bad and len(np.unique(codes[:, M - 1])) > 200                  # the late stages still choose
    # big: the largest e with (max |r|^2 + max |c|^2) 2^(2e) < 2^127 over the stages
    e = hq.big_exponent(oracle, x, cb)
    top = max((r.astype(np.float64) ** 2).sum(1).max() + (cb[m].astype(np.float64) ** 2).sum(1).max()
              for m, r in enumerate(hq.stage_residuals(oracle, x, cb)[:M]))
    assert top * 4.0 ** e < 2.0 ** 127 <= top * 4.0 ** (e + 1)
    assert e == 62 and e >= 60 and hq.rq_rung(oracle, "big", d, M)["e"] == e


@pytest.mark.parametrize("d,M", FUSED)
@pytest.mark.parametrize("name", ["big", "small"])
def test_big_and_small_are_exact_scalings(oracle, name, d, M):
    _, ctl = _enc(oracle, "unit", d, M)
    r, got = _enc(oracle, name, d, M)
    e = r["e"]
    assert np.array_equal(got[0], ctl[0]) and not got[3]
    assert np.array_equal(bits(got[1]), bits(md.scale(ctl[1], 2 * e)))
    assert np.array_equal(bits(got[2]), bits(md.scale(ctl[2], e)))
    assert np.all(got[1][got[1] > 0] >= TINY)                                 # nothing subnormal
    p = hq.pq_rung(oracle, name, d, 8)
    pc = hq.pq_rung(oracle, "unit", d, 8)
    a, b = pq_encode_ref(oracle, p["x"], p["cb"]), pq_encode_ref(oracle, pc["x"], pc["cb"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(md.scale(b[1], 2 * e))) and not a[2]


@pytest.mark.parametrize("d,M", FUSED)
def test_sub_keeps_the_codes_and_loses_bits(oracle, d, M):
    _, ctl = _enc(oracle, "unit", d, M)
    r, got = _enc(oracle, "sub", d, M)
    assert np.array_equal(got[0], ctl[0]) and not got[3]
    assert np.all(got[1][:, M - 1] < TINY)
    assert np.any(bits(got[1]) != bits(md.scale(ctl[1], -128)))


@pytest.mark.parametrize("d,M", FUSED)
def test_fade_reaches_zero_stage_by_stage(oracle, d, M):
    """The share of exact-zero distances is 0 at stage 0, never falls, grows strictly from the first stage that has any,
    and is above one half at the last stage (measured: 0, 0, 5.4 %, 80 % at d = 64; 0, 0, 8.8 %, 95 % at d = 128)."""
    _, ctl = _enc(oracle, "unit", d, M)
    r, got = _enc(oracle, "fade", d, M)
    share = (got[1] == 0).mean(0)
    assert share[0] == 0 and share[M - 1] > 0.5 and not got[3]
    for m in range(1, M):
        assert share[m] >= share[m - 1] and (share[m] > share[m - 1] or share[m] == 0), share
    assert share[M - 2] > 0
    assert (got[0] != ctl[0]).mean() >= 0.05


@pytest.mark.parametrize("d,M", FUSED + [(12, 3)])
def test_zero_is_all_code_0_at_plus_0(oracle, d, M):
    r, got = _enc(oracle, "zero", d, M)
    assert np.all(got[0] == 0) and np.all(bits(got[1]) == 0) and not got[3]
    p = hq.pq_rung(oracle, "zero", 64, 8)
    a = pq_encode_ref(oracle, p["x"], p["cb"])
    assert np.all(a[0] == 0) and np.all(bits(a[1]) == 0) and not a[2]


@pytest.mark.parametrize("B,n", [(5, hq.N), (32, 289)])
def test_zero_under_the_beam_is_the_all_ties_case(oracle, B, n):
    r = hq.rq_rung(oracle, "zero", 64, 3, n=n)
    st = rq_beam_step_ref(oracle, r["x"].reshape(n, 1, 64), 1, r["cb"][0], B)
    assert np.all(st[1] == 0) and np.array_equal(st[2], np.tile(np.arange(B, dtype=np.uint8), (n, 1)))   # (parent 0, word t)
    assert np.all(bits(st[3]) == 0) and not st[4]
    st2 = rq_beam_step_ref(oracle, st[0], B, r["cb"][1], B)                   # then (parent 0, word t) again: (D, slot, word)
    assert np.all(st2[1] == 0) and np.array_equal(st2[2], st[2]) and np.all(bits(st2[3]) == 0)
    codes, dist, _, bad = rq_beam_encode_ref(oracle, r["x"], r["cb"], B)
    assert np.all(codes == 0) and np.all(bits(dist) == 0) and not bad
    f = hq.rq_rung(oracle, "flat", 64, 3, n=n)
    sf = rq_beam_step_ref(oracle, f["x"].reshape(n, 1, 64), 1, f["cb"][0], B)
    # flat: every slot at +0 too, over the row's own set of tied words -- ascending, and not 0 .. B-1 for most rows
    assert np.all(bits(sf[3]) == 0) and np.all(np.diff(sf[2].astype(np.int64), axis=1) > 0) and np.all(sf[1] == 0)
    assert np.mean(sf[2][:, B - 1] != B - 1) > 0.5


@pytest.mark.parametrize("d,M", FUSED)
def test_unlisted_flags_exactly_the_planted_rows(oracle, d, M):
    r, got = _enc(oracle, "unlisted", d, M)
    codes, dist, res, bad = got
    over = np.zeros(hq.N, bool)
    over[r["overflow"]] = True
    assert bad and np.all(codes[over] == 0) and np.all(np.isposinf(dist[over]))          # at every stage
    assert np.all(np.isfinite(dist[~over]))
    assert set(r["overflow"]) >= {0, 31, 64, 95, hq.N - 1} and set(r["edge_sum"]) >= {32, 63, 96, 127}
    xn = (r["x"].astype(np.float64) ** 2).sum(1)
    assert np.all(xn[over] > 3.41e38) and np.all(np.isfinite(r["x"]))                    # finite elements, |x|^2 = +inf
    edge = np.zeros(hq.N, bool)
    edge[r["edge_sum"]] = True
    assert np.all(xn[edge] < 2e38) and np.all(xn[edge] > 1e38)
    cn = (r["cb"][0].astype(np.float64) ** 2).sum(1)
    assert np.all(cn[r["heavy"]] > 2.4e38) and np.all(cn[r["heavy"]] < 3.4e38) and np.all(cn[r["infnorm"]] > 3.41e38)
    assert not np.isin(codes[:, 0], r["infnorm"]).any() and not np.isin(codes[edge, 0], r["heavy"]).any()
    with np.errstate(all="ignore"):               # the NaN rows: xn + cn - 2 ip is inf - inf against every infnorm word
        P = ip_matrix(r["x"][r["nan_rows"]], r["cb"][0][r["infnorm"]])
        assert np.all(np.isposinf(P)) and np.all(np.isnan(np.float32(np.inf) - np.float32(2) * P)) and len(r["nan_rows"]) >= 9
    # every other row has the bits of the call without the planted rows
    clean = rq_encode_ref(oracle, r["x_clean"], r["cb"])
    keep = ~(over | edge)
    assert not clean[3] and np.array_equal(codes[keep], clean[0][keep])
    assert np.array_equal(bits(dist[keep]), bits(clean[1][keep])) and np.array_equal(bits(res[keep]), bits(clean[2][keep]))
    p = hq.pq_rung(oracle, "unlisted", d, 8)
    a = pq_encode_ref(oracle, p["x"], p["cb"])
    assert a[2] and np.all(np.isposinf(a[1][r["overflow"][::2], 0])) and not np.isin(a[0][:, 0], r["infnorm"]).any()


@pytest.mark.parametrize("d,M", FUSED)
@pytest.mark.parametrize("name", hq.OFF_NAMES)
def test_off_origin_rungs(oracle, name, d, M):
    """Stage 0 works at an offset of 100 (of up to 80 dB) with a spread s; from stage 1 on the offset is gone: every
    residual has a root-mean-square coordinate |r| / sqrt(d) of at most 4 s.  (The Euclidean norm itself is up to
    sqrt(2 d) s: the rows around the 20 centres whose centroid off_origin_data.build overwrites with a duplicate have no
    word nearer than another centre.)"""
    r, got = _enc(oracle, name, d, M)
    s = r["s"]
    zero0 = (got[1][:, 0] == 0).mean()
    assert not got[3]
    if name == "clamp":
        assert zero0 > 0.10
    if name == "flat":
        assert zero0 == 1.0
        T = md.true_sqdist(r["x"], r["cb"][0])
        assert (got[0][:, 0] == T.argmin(1)).mean() < 0.05                    # the contract's winner is not the fp64 one
    for q in hq.stage_residuals(oracle, r["x"], r["cb"])[1:]:
        assert np.sqrt((q.astype(np.float64) ** 2).sum(1) / d).max() <= 4 * s
    assert np.abs(r["x"].astype(np.float64).mean(0)).max() > 50           # while stage 0 sees the whole offset


@pytest.mark.parametrize("d", [64, 6])
def test_inner_product_rungs(oracle, d):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ctl = hq.ip_rung(oracle, "big", d)
        ids0, ip0 = search_ip_ref(ctl["x0"], ctl["c0"])
        for name in ("big", "small"):
            r = hq.ip_rung(oracle, name, d)
            ids, ip = search_ip_ref(r["x"], r["c"])
            assert np.array_equal(ids, ids0) and np.array_equal(bits(ip), bits(md.scale(ip0, 2 * r["e"])))
        r = hq.ip_rung(oracle, "sub", d)
        ids, ip = search_ip_ref(r["x"], r["c"])
        assert np.all(np.abs(ip) < TINY) and np.any(bits(ip) != bits(md.scale(ip0, -128))) and np.all(ids >= 0)
        # ipinf: several centroids at +inf, the lowest of them is the answer and not the control's arg-max
        r = hq.ip_rung(oracle, "ipinf", d)
        ids, ip = search_ip_ref(r["x"], r["c"])
        idsc, _ = search_ip_ref(r["x0"], r["c0"])
        P = ip_matrix(r["x"], r["c"])
        tied = (P == np.inf).sum(1) >= 2
        assert (tied & (ids != idsc)).sum() >= 20 and np.all(ids >= 0) and np.any(P == -np.inf)
        assert np.array_equal(ids[r["tie_rows"]], r["low"]) and np.array_equal(idsc[r["tie_rows"]], r["high"])
        assert np.all(ids[tied] == np.argmax(P[tied] == np.inf, axis=1))
        # zero: every product is +0 or -0 (a negative product that underflows rounds to -0, and fmaf(tiny, tiny, -0) with
        # another negative product keeps it: the sign is the last feature's); every row answers centroid 0, its own bits
        r = hq.ip_rung(oracle, "zero", d)
        ids, ip = search_ip_ref(r["x"], r["c"])
        P = ip_matrix(r["x"], r["c"])
        assert np.all(P == 0) and np.all(ids == 0) and np.array_equal(bits(ip), bits(P[:, 0]))
        assert np.any(bits(ip) == 0) and np.any(bits(ip) == 0x80000000)
        # neg: every product is negative, so the zero of a padded centroid would win
        r = hq.ip_rung(oracle, "neg", d)
        ids, ip = search_ip_ref(r["x"], r["c"])
        assert np.all(ip < 0) and np.all(ids >= 0) and np.all(ids < hq.IP_K) and hq.IP_K % 128 != 0


def test_spherical_training_is_scale_free(oracle):
    """k = 64, niter = 4, n = 4129: rows x 2^50 and x 2^-40 end with the control's centroid bits."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ctl = spherical_kmeans_ref(hq.spherical_rows(oracle, 0), 64, 4)
        for e in (50, -40):
            r = spherical_kmeans_ref(hq.spherical_rows(oracle, e), 64, 4)
            assert np.array_equal(bits(r.centroids), bits(ctl.centroids)) and r.nsplit == ctl.nsplit
            assert np.array_equal(r.assign, ctl.assign)


@pytest.mark.parametrize("d", [64, 6])
def test_renorm_rows_case(d):
    c = hq.renorm_rows_case(d)
    assert np.isfinite(c).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = renorm_ref(c)
        nr = np.zeros(10, np.float32)
        for f in range(d):
            nr = (c[:, f].astype(np.float64) ** 2 + nr).astype(np.float32)
    assert 0 < nr[0] < TINY and 0 < nr[1] < TINY and nr[2] == 0 and nr[3] == 0 and np.isposinf(nr[4]) and np.isposinf(nr[5])
    assert np.array_equal(bits(out[2]), bits(c[2])) and np.array_equal(bits(out[3]), bits(c[3]))
    assert np.all(out[4] == 0) and np.all(out[5] == 0) and np.array_equal(bits(out[7]), bits(c[7]))
    assert abs(np.linalg.norm(out[6].astype(np.float64)) - 1) < 1e-6


@pytest.mark.parametrize("d,M", [(64, 8), (128, 64)])
def test_pq_search_cases(oracle, d, M):
    k = 128
    seen_inf_sum = seen_short = seen_seam = False
    for name in ("big", "sub", "zero", "unlisted"):
        cs = hq.pq_search_case(oracle, name, d, M)
        codes = cs["codes"]
        assert codes.shape == (hq.NTOTAL, M) and len(np.unique(codes)) == 256
        assert np.array_equal(codes[hq.SLAB - 6:hq.SLAB + 10], codes[:16]) and np.array_equal(codes[:24], cs["own"])
        T = pq_tables(oracle, cs["x"], cs["cb"])
        dis, ok = pq_distances(T, codes)
        D, I = select(dis, ok, k)
        assert not np.isnan(D).any()
        if name == "zero":
            assert np.array_equal(I, np.tile(np.arange(k), (24, 1))) and np.all(bits(D) == 0)
            continue
        idx = codes.astype(np.int64)
        finite_terms = np.ones(dis.shape, bool)
        for m in range(M):
            finite_terms &= np.isfinite(T[:, m, :][:, idx[:, m]])
        seen_inf_sum |= bool((np.isposinf(dis) & finite_terms).any())
        short = (I < 0).any(1)
        if name == "unlisted":
            assert short.any()
            for i in np.flatnonzero(short):
                nl = int((I[i] >= 0).sum())
                assert np.all(I[i, nl:] == -1) and np.all(np.isposinf(D[i, nl:])) and np.all(np.isfinite(D[i, :nl]))
            seen_short = True
        else:
            assert not short.any() and np.array_equal(I[:, 0], np.arange(24))     # a query's own code row leads
        for i in range(24):
            for j in range(k - 1):
                if 0 <= I[i, j] < hq.SLAB <= I[i, j + 1] and bits(D[i, j:j + 1])[0] == bits(D[i, j + 1:j + 2])[0]:
                    seen_seam = True
        for i in range(16):
            if I[i, 0] == i and name != "unlisted":
                at = np.flatnonzero(I[i] == hq.SLAB - 6 + i)              # its copy follows, at the same distance
                assert at.size == 1 and at[0] >= 1 and bits(D[i, :1])[0] == bits(D[i, at[0]:at[0] + 1])[0]
    assert seen_inf_sum and seen_short and seen_seam
