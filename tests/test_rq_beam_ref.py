"""The beam-search residual quantiser without a GPU: tests/rq_beam_ref.py against an independent brute-force form and
against the greedy reference, its tie and non-finite rules, and the host logic of ops.ResidualQuantizer(max_beam_size=B)
on CPU stand-in backends whose beam stage is that reference (or whose knn() is tests/knn_ref.py)."""
import numpy as np
import pytest
import torch

from knn_ref import distance_matrix, knn_ref
from rq_beam_ref import (beam_widths, partial_fill_case, path_tie_case, rq_beam_encode_ref, rq_beam_step_ref)
from rq_ref import rq_encode_ref


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _books(seed, M, ksub, d):
    rng = np.random.default_rng(seed)
    cb = rng.standard_normal((M, ksub, d)).astype(np.float32)
    for m in range(M):
        cb[m] *= np.float32(0.5 ** m)
    return rng, cb


def _brute_step(oracle, r, b_in, book, b_out):
    """The full b_in * ksub candidate matrix and one lexsort per row: no truncation to k_m."""
    ksub, d = book.shape
    n = r.shape[0]
    dis, ok = distance_matrix(oracle, r.reshape(n * b_in, d), book)
    parent = np.zeros((n, b_out), np.int32)
    code = np.zeros((n, b_out), np.uint8)
    dist = np.full((n, b_out), np.inf, np.float32)
    ss, jj = np.divmod(np.arange(b_in * ksub), ksub)
    for i in range(n):
        di = dis[i * b_in:(i + 1) * b_in].ravel()
        keep = ok[i * b_in:(i + 1) * b_in].ravel() & (di < np.float32(np.inf))
        order = np.lexsort((jj[keep], ss[keep], di[keep]))[:b_out]
        parent[i, :order.size], code[i, :order.size] = ss[keep][order], jj[keep][order]
        dist[i, :order.size] = di[keep][order]
    r_out = r[np.arange(n)[:, None], parent] - book[code.astype(np.int64)]
    return np.ascontiguousarray(r_out), parent, code, dist, bool(np.isposinf(dist).any())


@pytest.mark.parametrize("n", [3, 30])
@pytest.mark.parametrize("d,ksub,B,M", [(8, 7, 3, 3), (16, 256, 5, 2)])
def test_reference_agrees_with_the_brute_force_form(oracle, d, ksub, B, M, n):
    rng, cb = _books(d + B, M, ksub, d)
    x = rng.standard_normal((n, d)).astype(np.float32)
    cb[:, ksub - 1] = cb[:, 1]                             # a duplicate word per stage: equal distances
    x[0] = cb[0, 1]
    got = rq_beam_encode_ref(oracle, x, cb, B)
    want = rq_beam_encode_ref(oracle, x, cb, B, step=_brute_step)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(bits(got[2]), bits(want[2])) and got[3] == want[3] and not got[3]
    r = x.reshape(n, 1, d)
    w = beam_widths(B, ksub, M)
    for m in range(M):
        a, b = rq_beam_step_ref(oracle, r, w[m], cb[m], w[m + 1]), _brute_step(oracle, r, w[m], cb[m], w[m + 1])
        for u, v in zip(a[:4], b[:4]):
            assert u.dtype == v.dtype and np.array_equal(u.view(np.uint8), v.view(np.uint8)), m
        assert np.all(a[3][:, 1:] >= a[3][:, :-1])         # slot 0 is the best
        r = a[0]


@pytest.mark.parametrize("n", [7, 19, 20, 200])
def test_a_beam_of_one_is_the_greedy_encoder(oracle, n):
    rng, cb = _books(5, 3, 256, 12)
    x = rng.standard_normal((n, 12)).astype(np.float32)
    x[2, 3] = np.nan
    got, want = rq_beam_encode_ref(oracle, x, cb, 1), rq_encode_ref(oracle, x, cb)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(bits(got[2]), bits(want[2])) and got[3] == want[3] and got[3]


def test_beam_widths_under_a_small_codebook(oracle):
    assert beam_widths(5, 3, 3) == [1, 3, 5, 5] and beam_widths(32, 256, 2) == [1, 32, 32] and beam_widths(4, 1, 3) == [1, 1, 1, 1]
    rng, cb = _books(3, 3, 3, 8)
    x = rng.standard_normal((25, 8)).astype(np.float32)
    r, seen = x.reshape(25, 1, 8), []
    for m, (b_in, b_out) in enumerate(((1, 3), (3, 5), (5, 5))):
        r, parent, code, dist, bad = rq_beam_step_ref(oracle, r, b_in, cb[m], b_out)
        seen.append(r.shape[1])
        assert not bad and np.all(np.isfinite(dist)) and parent.max() < b_in and code.max() < 3
    assert seen == [3, 5, 5]
    # stage 0 keeps all three words, nearest first
    _, _, code0, dist0, _ = rq_beam_step_ref(oracle, x.reshape(25, 1, 8), 1, cb[0], 3)
    D, I = knn_ref(oracle, x, cb[0], 3)
    assert np.array_equal(code0, I.astype(np.uint8)) and np.array_equal(bits(dist0), bits(D))


def test_path_ties_go_to_the_lower_parent_slot(oracle):
    x, cb, wa, wb, s = path_tie_case()
    n = x.shape[0]
    r1, p0, c0, d0, _ = rq_beam_step_ref(oracle, x.reshape(n, 1, -1), 1, cb[0], 3)
    assert np.array_equal(np.sort(c0[:, :2], 1), np.sort(np.stack([wa, wb], 1), 1))      # a and b lead stage 0
    r2, p1, c1, d1, _ = rq_beam_step_ref(oracle, r1, 3, cb[1], 3)
    assert np.array_equal(bits(d1[:, 0]), bits(d1[:, 1])) and np.all(d1[:, 2] > d1[:, 1])  # the tie, and only it
    assert np.all(p1[:, 0] == 0) and np.all(p1[:, 1] == 1)
    assert np.array_equal(c1[:, 0], c0[:, 1]) and np.array_equal(c1[:, 1], c0[:, 0])      # (a, b) and (b, a)
    assert np.array_equal(bits(r2[:, 0]), bits(s)) and np.array_equal(bits(r2[:, 1]), bits(s))
    codes, dist, res, bad = rq_beam_encode_ref(oracle, x, cb, 3)
    assert not bad and np.array_equal(codes[:, 0], c0[:, 0]) and np.array_equal(codes[:, 1], c0[:, 1])
    assert np.array_equal(bits(dist[:, 0]), bits(d0[:, 0])) and np.array_equal(bits(res), bits(s))


@pytest.mark.parametrize("n", [6, 40])
def test_a_nan_row_leaves_every_slot_unfilled(oracle, n):
    rng, cb = _books(8, 3, 256, 16)
    x = rng.standard_normal((n, 16)).astype(np.float32)
    clean = rq_beam_encode_ref(oracle, x, cb, 3)
    assert not clean[3]
    x[1, 5] = np.nan
    r_out, parent, code, dist, bad = rq_beam_step_ref(oracle, x.reshape(n, 1, 16), 1, cb[0], 3)
    assert bad and np.all(parent[1] == 0) and np.all(code[1] == 0) and np.all(np.isposinf(dist[1]))
    want = x[1] - cb[0, 0]                                 # every slot: parent 0's residual minus word 0
    assert all(np.array_equal(bits(r_out[1, s])[np.arange(16) != 5], bits(want)[np.arange(16) != 5]) for s in range(3))
    codes, dis, res, bad = rq_beam_encode_ref(oracle, x, cb, 3)
    assert bad and np.all(codes[1] == 0) and np.all(np.isposinf(dis[1])) and np.isnan(res[1, 5])
    keep = np.arange(n) != 1
    assert np.array_equal(codes[keep], clean[0][keep]) and np.array_equal(bits(dis[keep]), bits(clean[1][keep]))
    assert np.array_equal(bits(res[keep]), bits(clean[2][keep]))


@pytest.mark.parametrize("n", [30, 6])
def test_partial_fill_behind_the_filled_slots(oracle, n):
    x, book, row = partial_fill_case(n, 8)
    r_out, parent, code, dist, bad = rq_beam_step_ref(oracle, x.reshape(n, 1, 8), 1, book, 5)
    assert bad and list(code[row]) == [17, 99, 0, 0, 0]
    assert np.all(np.isfinite(dist[row, :2])) and np.all(np.isposinf(dist[row, 2:]))
    assert np.all(parent[row] == 0) and np.array_equal(bits(r_out[row, 2]), bits(x[row] - book[0]))
    assert np.array_equal(bits(r_out[row, 1]), bits(x[row] - book[99]))
    assert np.all(np.isfinite(dist[np.arange(n) != row]))   # the other rows list every word, however far


# ---- ops.ResidualQuantizer on CPU stand-ins -----------------------------------------------------------------------

def _stand_ins(oracle):
    from oracle_backend import OracleBackend

    class StepBackend(OracleBackend):
        """rq_beam_step is the reference."""
        def rq_beam_step(self, r, b_in, codebook, b_out):
            cb = self._f32(codebook).numpy()
            r_out, parent, code, dist, bad = rq_beam_step_ref(oracle, self._f32(r).numpy().reshape(-1, b_in, cb.shape[1]),
                                                              b_in, cb, b_out)
            return (torch.from_numpy(r_out), torch.from_numpy(parent), torch.from_numpy(code), torch.from_numpy(dist),
                    torch.tensor([int(bad)], dtype=torch.int32))

    class KnnBackend(OracleBackend):
        """Only knn(): ops composes the stage from it."""
        def knn(self, x, c, k, want_dist=True):
            D, I = knn_ref(oracle, self._f32(x).numpy(), self._f32(c).numpy(), k)
            return torch.from_numpy(I), torch.from_numpy(D)

    return OracleBackend, StepBackend, KnnBackend


@pytest.fixture(scope="module")
def table():
    rng, cb = _books(6, 3, 256, 16)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    cb[:, 200] = cb[:, 3]
    x[10:20] = cb[0, 3]
    return x, cb


def test_constructor_errors(oracle):
    from audio_tokens_amd.ops import ResidualQuantizer
    plain, step, knn = _stand_ins(oracle)
    for beam in (33, 100, 0, -1):
        with pytest.raises(NotImplementedError):
            ResidualQuantizer(16, 3, max_beam_size=beam, backend=step())
    with pytest.raises(NotImplementedError, match="rq_beam_step"):
        ResidualQuantizer(16, 3, max_beam_size=2, backend=plain())
    assert ResidualQuantizer(16, 3, max_beam_size=1, backend=plain()).max_beam_size == 1
    assert ResidualQuantizer(16, 3, max_beam_size=32, backend=step()).max_beam_size == 32
    assert ResidualQuantizer(16, 3, max_beam_size=5, backend=knn()).max_beam_size == 5


@pytest.mark.parametrize("which", ["step", "knn"])
@pytest.mark.parametrize("n", [300, 5, 0])
def test_compute_codes_against_the_reference(oracle, table, which, n):
    from audio_tokens_amd.ops import ResidualQuantizer
    _, step, knn = _stand_ins(oracle)
    x, cb = table
    x = x[:n]
    rq = ResidualQuantizer(16, 3, max_beam_size=3, backend=step() if which == "step" else knn())
    rq.set_centroids(cb)
    cr, dr, rr, bad = rq_beam_encode_ref(oracle, x, cb, 3)
    assert not bad
    codes = rq.compute_codes(x)
    assert isinstance(codes, np.ndarray) and codes.dtype == np.uint8 and codes.shape == (n, 3) and np.array_equal(codes, cr)
    codes2, dist, res = rq.compute_codes(x, return_distances=True, return_residual=True)
    assert np.array_equal(codes2, cr) and dist.dtype == np.float32 and np.array_equal(bits(dist), bits(dr))
    assert res.dtype == np.float32 and res.shape == (n, 16) and np.array_equal(bits(res), bits(rr))
    if n == 300:
        greedy = rq_encode_ref(oracle, x, cb)
        assert np.any(cr != greedy[0]) and dr[:, 2].sum() < greedy[1][:, 2].sum()   # (this table; no rule says so)
        assert np.array_equal(rq.compute_codes(x.astype(np.float64)), cr)           # float64: converted first
        wide = np.zeros((300, 32), np.float32)
        wide[:, ::2] = x
        c3, d3, r3 = rq.compute_codes(wide[:, ::2], return_distances=True, return_residual=True)
        assert np.array_equal(c3, cr) and np.array_equal(bits(d3), bits(dr)) and np.array_equal(bits(r3), bits(rr))
        tall = torch.zeros((600, 16))
        tall[::2] = torch.from_numpy(x)
        assert np.array_equal(rq.compute_codes(tall[::2]), cr)
        bad_x = x.copy()
        bad_x[7, 2] = np.inf
        with pytest.raises(RuntimeError, match="input contains NaN's or Inf's"):
            rq.compute_codes(bad_x)
        got = rq.compute_codes(bad_x, check_finite=False)
        assert np.all(got[7] == 0) and np.array_equal(np.delete(got, 7, 0), np.delete(cr, 7, 0))


def test_train_is_one_kmeans_per_stage_on_the_residuals_of_all_beams(oracle):
    from audio_tokens_amd.ops import ResidualQuantizer
    _, step, _ = _stand_ins(oracle)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((600, 16)).astype(np.float32)
    rq = ResidualQuantizer(16, 3, niter=3, max_beam_size=3, backend=step())
    rq.train(x)
    r, books, b = x.reshape(600, 1, 16), [], 1
    for m in range(3):
        books.append(oracle.kmeans_train(np.ascontiguousarray(r.reshape(-1, 16)), 256, niter=3).centroids)
        if m < 2:
            r = rq_beam_step_ref(oracle, r, b, books[-1], 3)[0]
            b = 3
    assert r.shape == (600, 3, 16)                          # stage 2 trained on 1800 rows
    assert rq.is_trained and np.array_equal(bits(rq.centroids), bits(np.stack(books)))
    greedy = ResidualQuantizer(16, 3, niter=3, backend=step())
    greedy.train(x)                                         # B = 1: today's training, another table from stage 1 on
    assert np.array_equal(bits(greedy.centroids[0]), bits(books[0])) and np.any(greedy.centroids[1] != books[1])
