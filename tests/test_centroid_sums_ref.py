"""tests/centroid_sums_ref.py (the reference the GPU centroid sums are held to) against the literal loop, on the CPU.

No GPU is needed.  test_finalize_is_the_oracle_backends loads the oracle's native library, as tests/test_knn_ref.py
does, so that one test needs a built tree; the others run on numpy alone."""
import numpy as np
import pytest
import torch

from centroid_sums_ref import finalize, ids_with_lengths, sequential_sums, sum_parts
from oracle_backend import OracleBackend


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _wide_rows(rng, n, d):
    """Rows scaled over 2^-8 .. 2^8: nearly every add rounds, so the order of the adds shows in the bits."""
    return (rng.standard_normal((n, d)) * np.exp2(rng.uniform(-8, 8, (n, 1)))).astype(np.float32)


@pytest.mark.parametrize("d", [1, 3, 8, 64])
def test_sequential_sums_is_the_literal_loop(d):
    rng = np.random.default_rng(100 + d)
    n, k = 3000, 7
    x = _wide_rows(rng, n, d)
    ids = rng.integers(0, k, n)
    ids[ids == 3] = 4                                   # an empty cluster
    ids[: n // 3] = 1                                   # and a heavy one
    bad = rng.choice(n, 40, replace=False)
    ids[bad[:20]] = -1
    ids[bad[20:]] = k + 2
    sums = np.zeros((k, d), np.float32)
    counts = np.zeros(k, np.float32)
    back = np.zeros((k, d), np.float32)
    for i in range(n):                                  # ascending row, fp32 adds
        if 0 <= ids[i] < k:
            sums[ids[i]] += x[i]
            counts[ids[i]] += 1
    for i in range(n - 1, -1, -1):
        if 0 <= ids[i] < k:
            back[ids[i]] += x[i]
    assert (bits(back) != bits(sums)).any()             # the data does tell the order of the adds
    got_sums, got_counts, order, sorted_ids = sequential_sums(x, ids, k)
    assert got_sums.dtype == np.float32 and got_counts.dtype == np.float32
    assert order.dtype == np.uint32 and sorted_ids.dtype == np.uint32
    assert np.array_equal(bits(got_sums), bits(sums))
    assert np.array_equal(bits(got_counts), bits(counts))
    key = np.where((ids >= 0) & (ids < k), ids, k)
    want = sorted(range(n), key=lambda i: (key[i], i))
    assert order.tolist() == want
    assert sorted_ids.tolist() == [int(key[i]) for i in want]
    assert counts[3] == 0 and not got_sums[3].any()


def test_ids_far_outside_go_to_the_trailing_bucket():
    k = 5
    ids = np.array([0, -1, 2**32, 2**32 + 2, 2, -2**63, 2**63 - 1, 2**31, k, 2], dtype=np.int64)
    x = np.arange(10, dtype=np.float32)[:, None] + 1
    sums, counts, order, sorted_ids = sequential_sums(x, ids, k)
    assert sums[:, 0].tolist() == [1.0, 0.0, 15.0, 0.0, 0.0] and counts.tolist() == [1.0, 0.0, 2.0, 0.0, 0.0]
    assert order.tolist() == [0, 4, 9, 1, 2, 3, 5, 6, 7, 8] and sorted_ids.tolist() == [0, 2, 2] + [k] * 7


def test_ids_with_lengths_yields_the_requested_bincount():
    rng = np.random.default_rng(5)
    lengths = np.array([0, 1, 2049, 0, 64, 65, 3, 0])
    ids, n = ids_with_lengths(lengths, rng)
    assert n == lengths.sum() and ids.dtype == np.int64 and ids.shape == (n,)
    assert np.array_equal(np.bincount(ids, minlength=lengths.size), lengths)
    rows = np.flatnonzero(ids == 2)
    assert rows[-1] - rows[0] + 1 > rows.size           # scattered: not one contiguous range of rows
    flat, _ = ids_with_lengths(lengths, rng, scatter=False)
    assert np.array_equal(flat, np.sort(ids))
    empty, n0 = ids_with_lengths(np.zeros(4, int), rng)
    assert n0 == 0 and empty.shape == (0,)


def test_finalize_is_the_oracle_backends():
    rng = np.random.default_rng(9)
    ob = OracleBackend()
    k, d, P = 6, 5, 3
    off, total = ob.part_layout(k, d)
    parts = np.zeros((P, total), np.float32)
    sums, counts = np.zeros((P, k, d), np.float32), np.zeros((P, k), np.float32)
    for p in range(P):
        x = _wide_rows(rng, 200, d)
        ids = rng.integers(0, k, 200)
        ids[ids == 2] = 1                               # cluster 2 empty in every part
        if p != 1:
            ids[ids == 4] = 5                           # cluster 4 empty in all parts but one
        sums[p], counts[p], _, _ = sequential_sums(x, ids, k)
        parts[p, : k * d] = sums[p].ravel()
        parts[p, k * d: k * d + k] = counts[p]
        parts[p, off:] = 7.0                            # (the objective slot: not part of the sums)
    cent, cnt = finalize(sums, counts)
    cent_o, cnt_o = ob.centroid_finalize(torch.from_numpy(parts), k, d)
    assert np.array_equal(bits(cent), bits(cent_o.numpy())) and np.array_equal(bits(cnt), bits(cnt_o.numpy()))
    assert cnt[2] == 0 and not cent[2].any() and (counts[:, 4] == 0).sum() == P - 1
    assert np.array_equal(bits(sum_parts(parts)), bits(ob.sum_parts(torch.from_numpy(parts)).numpy()))
    # one part: the sum scaled by the reciprocal, not divided
    c1, _ = finalize(sums[:1], counts[:1])
    nz = counts[0] > 0
    assert np.array_equal(bits(c1[nz]), bits(sums[0][nz] * (np.float32(1) / counts[0][nz])[:, None]))
