"""Hard data for the quantisers and the inner-product routes: the rungs of tests/test_hard_quantiser_ref.py and
tests/test_gpu_hard_quantisers.py.  The scaling and the base table are tests/magnitude_data.py's, the off-origin ladder
is tests/off_origin_data.py's; nothing of either is copied here.

Residual quantiser (rq_rung): stage m of the control holds ksub unit-norm words x 2^-m (words 0 .. 19 repeated at
ksub/2 .. ksub/2 + 19), rows are a sum of one word per stage + 0.02 x a unit row, the first 64 rows exactly such a sum.

    unit      the control
    big       rows and every codebook x 2^e, e the largest power for which the control's largest xn + cn stays < 2^127
    small     x 2^-40
    sub       x 2^-64: the late stages' distances are subnormal
    fade      x 2^-70: the residual reaches zero stage by stage
    zero      x 2^-80: every distance +0, every code 0
    unlisted  the control plus magnitude_data.rung("unlisted")'s planted rows and words, at its positions; every fourth
              overflowing row also meets the words of norm^2 +inf at a NaN (inf - inf) instead of +inf
    far, clamp, flat, db   stage 0 = the ksub centroids of off_origin_data.build at the rung's offset and spread s, and
              its rows (every row near a word); stages 1 .. are the control's, scaled by s

Product quantiser (pq_rung): the stage-0 table of the same rung cut into M contiguous slices.
Inner product (ip_rung): magnitude_data.base at k = 300, scaled; see ip_rung.
PQ search (pq_search_case): 24 queries of a rung against a database of two slabs.

TEST ONLY."""
import functools

import numpy as np

import magnitude_data as md
import off_origin_data as ood

N = 1057                     # 33 tiles of 32 rows + one row
ON_SUM = 64                  # the first rows sit exactly on a sum of words
SCALED = {"small": -40, "sub": -64, "fade": -70, "zero": -80}
SCALED_NAMES = ("big", "small", "sub", "fade", "zero")
OFF_NAMES = ("far", "clamp", "flat", "db")
IP_EXP = {"unit": 0, "big": 60, "ipinf": 64, "small": -40, "sub": -64, "zero": -80}
IP_NAMES = ("big", "ipinf", "small", "sub", "zero", "neg")
IP_K = 300
N_TIE = 40                   # ipinf: planted rows with two centroids at +inf
Q_ROWS = np.array([0, 31, 32, 63, 64, 65, 96, 97] + list(range(128, 144)))     # the 24 queries of a PQ search case
SLAB = 65536
NTOTAL = SLAB + 300
INF = np.float32(np.inf)


def _unit(rng, n, d, oracle):
    return oracle.l2norm_rows(rng.standard_normal((n, d)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def rq_table(oracle, seed, n, d, M, ksub=256):
    """The control: (x [n, d], codebooks [M, ksub, d], pick [n, M]) float32."""
    rng = np.random.default_rng(seed)
    cb = np.empty((M, ksub, d), np.float32)
    nd = min(20, ksub // 4)
    for m in range(M):
        w = _unit(rng, ksub, d, oracle)
        w[ksub // 2: ksub // 2 + nd] = w[0:nd]
        cb[m] = md.scale(w, -m)                    # exact
    pick = rng.integers(0, ksub, (n, M))
    x = np.zeros((n, d), np.float32)
    for m in range(M):
        x = x + cb[m][pick[:, m]]
    noise = np.float32(0.02) * _unit(rng, n, d, oracle)
    x[ON_SUM:] = x[ON_SUM:] + noise[ON_SUM:]
    assert x.dtype == np.float32
    return np.ascontiguousarray(x), cb, pick


def stage_residuals(oracle, x, cb):
    """[M + 1] list of the greedy residual in front of every stage (and behind the last)."""
    r, out = np.ascontiguousarray(x, dtype=np.float32), []
    with np.errstate(all="ignore"):
        for m in range(cb.shape[0]):
            out.append(r)
            ids, _ = oracle.assign(r, cb[m])
            r = np.ascontiguousarray(r - cb[m][np.maximum(ids, 0)], dtype=np.float32)
    out.append(r)
    return out


def big_exponent(oracle, x, cb):
    """The largest e with max over the stages of (max |r|^2 + max |c|^2) x 2^(2e) < 2^127 (float64 norms)."""
    res = stage_residuals(oracle, x, cb)
    top = max((res[m].astype(np.float64) ** 2).sum(1).max() + (cb[m].astype(np.float64) ** 2).sum(1).max()
              for m in range(cb.shape[0]))
    e = 0
    while top * 4.0 ** (e + 1) < 2.0 ** 127:
        e += 1
    return e


@functools.lru_cache(maxsize=None)
def rq_rung(oracle, name, d, M, ksub=256, n=N, seed=9):
    """dict(x, cb, e; unlisted: overflow, edge_sum, heavy, infnorm, nan_rows, x_clean; off-origin: s)."""
    x, cb, _ = rq_table(oracle, seed, n, d, M, ksub)
    out = {"e": None}
    if name == "unit":
        out["e"] = 0
    elif name == "big" or name in SCALED:
        e = big_exponent(oracle, x, cb) if name == "big" else SCALED[name]
        x, cb = md.scale(x, e), md.scale(cb, e)
        out["e"] = e
    elif name == "unlisted":
        assert ksub == 256
        u = md.rung(oracle, "unlisted", d, ksub, n=n, seed=seed)
        out.update(overflow=u["overflow"], edge_sum=u["edge_sum"], heavy=u["heavy"], infnorm=u["infnorm"], x_clean=x)
        x, cb = x.copy(), cb.copy()
        planted = np.concatenate([u["overflow"], u["edge_sum"]])
        x[planted] = u["x"][planted]
        cb[0][u["heavy"]] = u["c"][u["heavy"]]
        cb[0][u["infnorm"]] = u["c"][u["infnorm"]]
        # every fourth overflowing row is large in the infnorm words' own feature too: its product with them is +inf, and
        # |x|^2 + |c|^2 - 2 (+inf) is a NaN, not +inf -- a clamp that turns a NaN into 0 would list those words at 0
        nan_rows = u["overflow"][::4]
        x[nan_rows, 1] = np.float32(2e19)
        out["nan_rows"] = nan_rows
    elif name in OFF_NAMES:
        A, s = ood.RUNGS[d if d in ood.RUNGS else 64][name]
        xo, co = ood.build(seed, n, ksub, d, A, s)          # (every row is near a word: see DESIGN 5.0g on k = 1000)
        cb = cb.copy()
        cb[0] = co
        cb[1:] = (cb[1:] * np.float32(s)).astype(np.float32)
        x = xo
        out["s"] = s
    else:
        raise KeyError(name)
    assert np.isfinite(x).all() and np.isfinite(cb).all()
    out.update(x=np.ascontiguousarray(x), cb=np.ascontiguousarray(cb))
    return out


def pq_books(book, M):
    """[ksub, d] -> [M, ksub, d / M]: the contiguous slices of one table."""
    dsub = book.shape[1] // M
    return np.ascontiguousarray(np.stack([book[:, m * dsub:(m + 1) * dsub] for m in range(M)]))


@functools.lru_cache(maxsize=None)
def pq_rung(oracle, name, d, M, n=N, seed=9):
    """dict(x, cb [M, 256, d / M], e, and rq_rung's index sets): the one-stage table of the rung, sliced."""
    r = dict(rq_rung(oracle, name, d, 1, 256, n, seed))
    r["cb"] = pq_books(r["cb"][0], M)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# inner product

def ip_table(oracle, seed, n, d, k):
    return md.base(oracle, seed, n, d, k)


@functools.lru_cache(maxsize=None)
def ip_rung(oracle, name, d, k=IP_K, n=N, seed=9):
    """dict(x, c, x0, c0): the rung and its control (the same table unscaled).
        big, small, sub, zero   rows and centroids x 2^e each
        ipinf    x 2^64 each, with a plant: rows n - 40 .. n - 1 are 1.03 x a centroid b = 250 + t % 20; centroid 40 + t is
                 b / 1.015 (the control's runner-up, at +inf too and the lower index), centroid 60 + t is -b (-inf)
        neg      rows |x|, centroids -|c| x 2^-80: every product is negative and tiny, nothing but padding is at 0"""
    x, c = ip_table(oracle, seed, n, d, k)
    out = {}
    if name == "ipinf":
        x, c = x.copy(), c.copy()
        t = np.arange(20)
        c[250 + t] = (c[250 + t] * np.float32(1.015625)).astype(np.float32)
        c[40 + t] = (c[250 + t] * np.float32(0.984375)).astype(np.float32)
        c[60 + t] = -c[250 + t]
        rows = np.arange(n - N_TIE, n)
        x[rows] = (c[250 + np.arange(N_TIE) % 20] * np.float32(1.015625)).astype(np.float32)
        out.update(tie_rows=rows, low=40 + np.arange(N_TIE) % 20, high=250 + np.arange(N_TIE) % 20)
    if name == "neg":
        x, c = np.abs(x) + np.float32(0.01), -(np.abs(c) + np.float32(0.01))
        out.update(x0=x, c0=c, x=x, c=md.scale(c, IP_EXP["zero"]))
    else:
        e = IP_EXP[name]
        out.update(x0=x, c0=c, x=md.scale(x, e), c=md.scale(c, e), e=e)
    assert all(np.isfinite(out[key]).all() for key in ("x", "c"))
    return out


def spherical_rows(oracle, e, n=4129, d=64, k=64, seed=9):
    """Rows for Kmeans(spherical=True): magnitude_data.base's rows x 2^e."""
    return md.scale(md.base(oracle, seed, n, d, k)[0], e)


def renorm_rows_case(d=64):
    """Rows for at_renorm_rows_f32 whose norm^2 is subnormal, +inf from finite elements, exactly 0 (from elements whose
    squares vanish, and from zeros), and ordinary -> [10, d] float32."""
    rng = np.random.default_rng(d)
    c = rng.standard_normal((10, d)).astype(np.float32)
    c[0] = md.scale(c[0], -68)                     # norm^2 ~ d 2^-136: subnormal
    c[1] = md.scale(c[1], -72)                     # deeper: a few bits left
    c[2] = md.scale(c[2], -80)                     # every square vanishes: norm^2 = +0, the row stays
    c[3] = 0.0
    c[4] = np.float32(2.4e18)                      # +inf only from the sum when d >= 64; from fewer, larger elements below
    c[5] = 0.0
    c[5, d // 2] = np.float32(2e19)                # one square overflows
    c[6] = md.scale(c[6], 60)                      # large, finite
    c[7] = -0.0
    if d < 64:
        c[4] = np.float32(1.5e19)
    return np.ascontiguousarray(c)


# ---------------------------------------------------------------------------------------------------------------------
# PQ search

@functools.lru_cache(maxsize=None)
def pq_search_case(oracle, name, d, M, seed=9):
    """dict(x [24, d], cb [M, 256, d / M], codes [NTOTAL, M] uint8, own [24, M]).  The codes are the same on every rung:
    rows 0 .. 23 are the control's codes of the 24 queries, rows 24 .. 39 use `heavy` words only (magnitude_data's
    unlisted words 200 .. 215), rows 100 .. 355 are word j in every sub-space, the rest is drawn; rows SLAB - 6 ..
    SLAB + 9 are copies of rows 0 .. 15: exact ties across the slab seam."""
    from pq_ref import pq_encode_ref
    ctl = pq_rung(oracle, "unit", d, M, seed=seed)
    r = pq_rung(oracle, name, d, M, seed=seed)
    own = pq_encode_ref(oracle, ctl["x"][Q_ROWS], ctl["cb"])[0]
    rng = np.random.default_rng(seed + 5)
    codes = rng.integers(0, 256, (NTOTAL, M)).astype(np.uint8)
    codes[:24] = own
    codes[24:40] = np.arange(200, 216, dtype=np.uint8)[:, None]
    codes[100:356] = np.arange(256, dtype=np.uint8)[:, None]
    codes[SLAB - 6: SLAB + 10] = codes[0:16]
    assert len(np.unique(codes)) == 256
    out = dict(r)
    out.update(x=np.ascontiguousarray(r["x"][Q_ROWS]), codes=codes, own=own)
    return out
