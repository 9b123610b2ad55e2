"""CPU reference of the beam-search residual quantiser (ops.ResidualQuantizer(max_beam_size=B), at_rq_beam_step_f32 /
at_rq_beam_encode_f32): tests/knn_ref.py's search over the residuals of all beams as ONE call per stage, np.lexsort on
(D, parent slot, word), numpy float32 subtraction.  No float64 anywhere.  TEST ONLY."""
import numpy as np

from knn_ref import knn_ref

INF = np.float32(np.inf)


def beam_widths(beam, ksub, M):
    """[B_0, ..., B_M]: B_0 = 1, B_{m+1} = min(beam, B_m * ksub)."""
    w = [1]
    for _ in range(M):
        w.append(min(beam, w[-1] * ksub))
    return w


def select_ref(D, I, n, b_in, b_out):
    """The b_out smallest candidates of every row by (D, s, I) from the lists D, I [n * b_in, k] (id -1: nothing listed)
    -> (parent int32, code uint8, dist float32) [n, b_out]; unfilled slots: parent 0, code 0, +inf."""
    k = D.shape[1]
    parent = np.zeros((n, b_out), np.int32)
    code = np.zeros((n, b_out), np.uint8)
    dist = np.full((n, b_out), INF, np.float32)
    slot = np.repeat(np.arange(b_in), k)
    for i in range(n):
        di, ii = D[i * b_in:(i + 1) * b_in].ravel(), I[i * b_in:(i + 1) * b_in].ravel()
        keep = ii >= 0
        di, ii, si = di[keep], ii[keep], slot[keep]
        order = np.lexsort((ii, si, di))[:b_out]
        parent[i, :order.size], code[i, :order.size], dist[i, :order.size] = si[order], ii[order], di[order]
    return parent, code, dist


def rq_beam_step_ref(oracle, r, b_in, book, b_out):
    """r [n, b_in, d] (or [n * b_in, d]), book [ksub, d] -> (r_out float32 [n, b_out, d], parent int32, code uint8, dist
    float32 [n, b_out], bad bool).  The lists are knn_ref over all n * b_in residuals in one call (its direct form when
    n * b_in < 20) with k = min(b_out, ksub)."""
    book = np.ascontiguousarray(book, dtype=np.float32)
    ksub, d = book.shape
    r = np.ascontiguousarray(r, dtype=np.float32).reshape(-1, b_in, d)
    n = r.shape[0]
    assert 1 <= b_out <= b_in * ksub
    if n == 0:
        z = np.zeros((0, b_out))
        return np.zeros((0, b_out, d), np.float32), z.astype(np.int32), z.astype(np.uint8), z.astype(np.float32), False
    with np.errstate(all="ignore"):
        D, I = knn_ref(oracle, r.reshape(n * b_in, d), book, min(b_out, ksub))
        parent, code, dist = select_ref(D, I, n, b_in, b_out)
        r_out = r[np.arange(n)[:, None], parent] - book[code.astype(np.int64)]
    assert r_out.dtype == np.float32
    return np.ascontiguousarray(r_out), parent, code, dist, bool(np.isposinf(dist).any())


def trace_ref(steps):
    """steps: the (parent, code, dist) of every stage -> (codes uint8 [n, M], dist float32 [n, M]) of slot 0's path."""
    n = steps[0][0].shape[0]
    rows, slot = np.arange(n), np.zeros(n, np.int64)
    codes = np.zeros((n, len(steps)), np.uint8)
    dist = np.zeros((n, len(steps)), np.float32)
    for m in range(len(steps) - 1, -1, -1):
        parent, code, dis = steps[m]
        codes[:, m], dist[:, m] = code[rows, slot], dis[rows, slot]
        slot = parent[rows, slot].astype(np.int64)
    return codes, dist


def rq_beam_encode_ref(oracle, x, codebooks, beam, step=rq_beam_step_ref):
    """x [n, d], codebooks [M, ksub, d] -> (codes uint8 [n, M], dist float32 [n, M], residual float32 [n, d], bad bool):
    the path, the distances along it and the residual of slot 0 behind the last stage."""
    codebooks = np.ascontiguousarray(codebooks, dtype=np.float32)
    M, ksub, d = codebooks.shape
    r = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 1, d)
    n = r.shape[0]
    if n == 0:
        return np.zeros((0, M), np.uint8), np.zeros((0, M), np.float32), np.zeros((0, d), np.float32), False
    w = beam_widths(beam, ksub, M)
    steps, bad = [], False
    for m in range(M):
        r, parent, code, dist, bad_m = step(oracle, r, w[m], codebooks[m], w[m + 1])
        steps.append((parent, code, dist))
        bad = bad or bad_m
    codes, dist = trace_ref(steps)
    return codes, dist, np.ascontiguousarray(r[:, 0]), bad


def path_tie_case(n=64, d=8, ksub=256, seed=2):
    """Codebook 0 == codebook 1 on a dyadic grid: small words (entries -1, 0, 1) and the big words 8 e_f at index
    10 + 20 f (f < 8).  A row a + b + s of two different big words and a small dyadic s has a and b as its two nearest
    stage-0 words, and the paths (a, b) and (b, a) leave the residual s exactly: the two best stage-1 candidates tie in D.
    -> (x [n, d], codebooks [2, ksub, d], word a, word b, s)"""
    rng = np.random.default_rng(seed)
    book = rng.integers(-1, 2, (ksub, d)).astype(np.float32)
    big = 10 + 20 * np.arange(8)
    book[big] = 0
    book[big, np.arange(8)] = 8
    ia = rng.integers(0, 8, n)
    ib = (ia + rng.integers(1, 8, n)) % 8
    s = rng.integers(-1, 2, (n, d)).astype(np.float32) * np.float32(0.125)
    x = book[big[ia]] + book[big[ib]] + s
    return np.ascontiguousarray(x), np.stack([book, book]), big[ia], big[ib], s


def partial_fill_case(n, d, seed=9, row=4):
    """A row of 3.5e18 in 8 features (|x|^2 about 1e38, finite) and a codebook whose words are -x (1 + j 2^-12) but for
    the ordinary words 17 and 99: the row's distance to those two is about 1e38, every other one overflows (4e38), in the
    expansion form and in the direct one.  The ordinary rows list every word, the big ones far away but finite.
    -> (x [n, d], book [256, d], row)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[row] = 0
    x[row, :8] = np.float32(3.5e18)
    book = np.empty((256, d), np.float32)
    for j in range(256):
        book[j] = -x[row] * np.float32(1 + j * 2.0 ** -12)
    book[17] = rng.standard_normal(d).astype(np.float32)
    book[99] = book[17] + np.float32(1.0)                  # (at 1e38 the row sees both at the same distance: word 17 first)
    return x, book, row
