"""CPU reference of the greedy residual quantiser (ops.ResidualQuantizer, at_rq_encode_f32 / at_rq_decode_f32): numpy
float32 and the oracle's nearest-centroid search, one call per stage on the running residual.  No float64 anywhere.
TEST ONLY."""
import numpy as np


def rq_encode_ref(oracle, x, codebooks):
    """x [n, d], codebooks [M, ksub, d] -> (codes uint8 [n, M], dist float32 [n, M], residual float32 [n, d], bad
    bool).  Stage m is oracle.assign on the residual against codebooks[m] (its direct form when n < 20); where it lists
    nothing (id -1: no distance below +inf) the code is 0, the distance +inf, and bad is set; then every row subtracts
    its word, one float32 subtraction per feature."""
    r = np.ascontiguousarray(x, dtype=np.float32).copy()
    codebooks = np.ascontiguousarray(codebooks, dtype=np.float32)
    n, d = r.shape
    M, ksub, dc = codebooks.shape
    assert dc == d and 1 <= ksub <= 256
    codes = np.zeros((n, M), np.uint8)
    dist = np.full((n, M), np.inf, np.float32)
    bad = False
    if n == 0:
        return codes, dist, r, bad
    with np.errstate(all="ignore"):
        for m in range(M):
            ids, dis = oracle.assign(r, codebooks[m])
            none = ids < 0
            bad = bad or bool(none.any())
            codes[:, m] = np.where(none, 0, ids).astype(np.uint8)
            dist[:, m] = np.where(none, np.float32(np.inf), dis)
            r = np.ascontiguousarray(r - codebooks[m][codes[:, m].astype(np.int64)], dtype=np.float32)
    assert r.dtype == np.float32
    return codes, dist, r, bad


def rq_decode_ref(codes, codebooks):
    """codes uint8 [n, M], codebooks [M, ksub, d] -> float32 [n, d]: word codes[:, 0] of codebook 0 copied, then the
    words of the codebooks 1 .. M-1 added in ascending order, one float32 addition each."""
    codebooks = np.ascontiguousarray(codebooks, dtype=np.float32)
    idx = np.asarray(codes).astype(np.int64)
    out = codebooks[0][idx[:, 0]].copy()
    with np.errstate(all="ignore"):
        for m in range(1, codebooks.shape[0]):
            out = out + codebooks[m][idx[:, m]]
    assert out.dtype == np.float32
    return out
