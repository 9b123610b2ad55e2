"""CPU reference of the product quantiser (ops.ProductQuantizer, at_pq_encode_f32 / at_pq_decode_f32): numpy and the
oracle's nearest-centroid search, one call per sub-space.  TEST ONLY."""
import numpy as np


def pq_encode_ref(oracle, x, codebooks):
    """x [n, d], codebooks [M, ksub, dsub] -> (codes uint8 [n, M], dist float32 [n, M], bad bool).  Sub-space m is
    oracle.assign on the contiguous slice m of x against codebooks[m] (its direct form when n < 20); where it lists
    nothing (id -1: no distance below +inf) the code is 0, the distance +inf, and bad is set."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    codebooks = np.ascontiguousarray(codebooks, dtype=np.float32)
    n, d = x.shape
    M, ksub, dsub = codebooks.shape
    assert M * dsub == d and 1 <= ksub <= 256
    codes = np.zeros((n, M), np.uint8)
    dist = np.full((n, M), np.inf, np.float32)
    bad = False
    if n == 0:
        return codes, dist, bad
    for m in range(M):
        ids, dis = oracle.assign(np.ascontiguousarray(x[:, m * dsub:(m + 1) * dsub]), codebooks[m])
        none = ids < 0
        bad = bad or bool(none.any())
        codes[:, m] = np.where(none, 0, ids).astype(np.uint8)
        dist[:, m] = np.where(none, np.float32(np.inf), dis)
    return codes, dist, bad


def pq_decode_ref(codes, codebooks):
    """codes uint8 [n, M], codebooks [M, ksub, dsub] -> float32 [n, M * dsub]: the codebook rows, copied."""
    codebooks = np.ascontiguousarray(codebooks, dtype=np.float32)
    M, _, dsub = codebooks.shape
    out = np.empty((codes.shape[0], M * dsub), np.float32)
    for m in range(M):
        out[:, m * dsub:(m + 1) * dsub] = codebooks[m][codes[:, m].astype(np.int64)]
    return out
