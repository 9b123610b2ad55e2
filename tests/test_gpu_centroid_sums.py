"""at_centroid_accum_f32 on the MI355X against tests/centroid_sums_ref.py, bit for bit: every member-list length at which
a loop of csrc/accum.hip changes course, every vector width and alignment of the plan, the sizes at which the strategy
flips, ids and row values that must not be mistaken, and sequences of calls on one context (the predictions, generation
marks, bucket counters and workspaces a call inherits from the one before).

Every comparison is on bit patterns; where a NaN is expected the NaN masks are compared and the bits elsewhere.  Every
call writes into a result buffer filled with NaN beforehand, so a sum that no kernel wrote shows as a difference.
Where accum_plan forces the strategy (k > 16384, n > 64 k, d % 4 != 0, unaligned rows) the case id says so."""
import functools

import numpy as np
import pytest
import torch

from centroid_sums_ref import finalize, ids_with_lengths, sequential_sums, sum_parts
from device_rows import rows_one_float_off

pytestmark = pytest.mark.gpu

LONG_LIST = 2048     # accum_plan's long_list: longer member lists go to centroid_accum_long_kernel
EARLY_MAX = 16       # long clusters served by the ordered compaction
BOTH = [pytest.param(1, id="buckets"), pytest.param(0, id="sort")]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, ref, nan_ok, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    differ = bits(got) != bits(ref)
    if nan_ok:
        gn, rn = np.isnan(got), np.isnan(ref)
        assert np.array_equal(gn, rn), f"{what}: NaN masks differ, first at {np.argwhere(gn != rn)[0]}"
        differ &= ~rn
    bad = np.argwhere(differ)
    assert bad.size == 0, (f"{what}: {len(bad)} of {got.size} values differ, first at {bad[0]}: "
                           f"got {got[tuple(bad[0])]!r} want {ref[tuple(bad[0])]!r}")


def _wide_rows(rng, n, d, lo=-8, hi=8):
    """Rows scaled over 2^lo .. 2^hi: nearly every add rounds, so any reordering of the adds shows in the bits."""
    x = rng.random((n, d), dtype=np.float32)             # (uniform: a third of the time of standard_normal at 190 000 x 640)
    x -= np.float32(0.5)
    x *= np.exp2(rng.uniform(lo, hi, (n, 1))).astype(np.float32)
    return x


def _rows_dev(be, x, aligned=True):
    """x on the device: 16-byte aligned, or -- the plan's other branch -- a contiguous view one float behind that."""
    if aligned:
        t = be._f32(x)
        assert t.data_ptr() % 16 == 0
        return t
    return rows_one_float_off(x, be.device)


def _ids_dev(be, ids):
    return torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(be.device)


def _out(be, k, d, extra=0):
    return torch.full((k * d + k + extra,), float("nan"), dtype=torch.float32, device=be.device)


def _verify(be, got, ref, k, d, want_order=True, nan_ok=False, label=""):
    sums, counts, r_order, r_sorted = ref
    part, pair = got if want_order else (got, None)
    p = part.cpu().numpy()
    _same(p[: k * d].reshape(k, d), sums, nan_ok, f"{label}: sums")
    _same(p[k * d: k * d + k], counts, False, f"{label}: counts")
    if want_order:
        nv = int((r_sorted < k).sum())
        order = pair[0].cpu().numpy().view(np.uint32)
        assert np.array_equal(order[:nv], r_order[:nv]), f"{label}: member order"
        assert np.array_equal(np.sort(order[nv:]), np.sort(r_order[nv:])), f"{label}: trailing bucket"
        assert np.array_equal(pair[1].cpu().numpy().view(np.uint32), r_sorted), f"{label}: sorted ids"
    cent, h = be.centroid_finalize(part[: k * d + k], k, d)
    r_cent, r_h = finalize(sums[None], counts[None])
    _same(cent.cpu().numpy(), r_cent, nan_ok, f"{label}: finalize")
    _same(h.cpu().numpy(), r_h, False, f"{label}: hassign")


def _check(be, x, xt, ids, k, label, want_order=True, nan_ok=False, ref=None):
    """One call against the reference -> the reference."""
    d = x.shape[1]
    if ref is None:
        ref = sequential_sums(x, ids, k)
    got = be.centroid_accum(xt, _ids_dev(be, ids), k, out=_out(be, k, d), want_order=want_order)
    _verify(be, got, ref, k, d, want_order, nan_ok, label)
    return ref


def _known_state(be, switches):
    """A call per strategy with a k that nothing else uses: whatever an earlier test left in the session's context,
    the predictions, generation marks and bucket counters are now laid out (and cleared) for that k."""
    k, n, d = 4441, 2100, 4
    rng = np.random.default_rng(4441)
    x = _wide_rows(rng, n, d)
    ids = np.full(n, 17, np.int64)
    ids[:40] = 4000
    xt = _rows_dev(be, x)
    for b in (0, 1):
        switches(accum_buckets=b)
        _check(be, x, xt, ids, k, f"known state, accum_buckets={b}")


def _ids_with_long(rng, n, k, long, empty=()):
    """n ids: cluster c has long[c] members for the named ones (whatever their lengths), none for `empty`, the rest of
    the rows spread over the other clusters, none of which is long."""
    lengths = np.zeros(k, np.int64)
    others = np.setdiff1d(np.arange(k), np.array(list(long) + list(empty), dtype=np.int64))
    rest = n - sum(long.values())
    assert rest >= 0
    lengths[others] = rng.multinomial(rest, np.full(others.size, 1.0 / others.size))
    assert lengths.max() <= LONG_LIST
    for c, m in long.items():
        lengths[c] = m
    ids, n_ = ids_with_lengths(lengths, rng)
    assert n_ == n
    return ids


def _skewed_ids(rng, n, k, n_long, share=0.6):
    ids = rng.integers(0, k, n)
    heavy = rng.choice(k, n_long, replace=False)
    pick = rng.random(n) < share
    ids[pick] = heavy[rng.integers(0, n_long, int(pick.sum()))]
    counts = np.bincount(ids, minlength=k)
    assert int((counts > LONG_LIST).sum()) == n_long
    return ids


@pytest.fixture(scope="module", autouse=True)
def _release_cached_cases():
    """The cached cases (up to 450 MB of rows) are let go when this file is done, not kept for the rest of the session."""
    yield
    for cached in (_ladder_ids, _ladder_case, _largest_table_case):
        cached.cache_clear()


# ---- a. the length ladder -------------------------------------------------------------------------------------------
SHORT = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 79, 80, 81, 127, 128, 129, 191, 192, 193,
         1023, 1024, 1025, 2047, 2048]
LONG = [2049, 2050, 4095, 4096, 4097, 6143, 6144, 6145]
LONG_TAILS = [2 * 2048 + t for t in (15, 16, 17, 127, 128, 129, 143, 144, 145)]
LADDER = SHORT + LONG + LONG_TAILS
K_LADDER = 3000
LADDER_D = [1, 2, 3, 4, 6, 8, 64, 65, 66, 128, 130, 252, 256, 258, 260, 640]


@functools.lru_cache(maxsize=1)
def _ladder_ids():
    rng = np.random.default_rng(2048)
    k = K_LADDER
    lengths = rng.integers(0, 201, k) * (rng.random(k) < 0.3)          # filler clusters: 0 .. 200 members
    slots = np.concatenate([[0, k - 1], 1 + rng.choice(k - 2, len(LADDER) - 2, replace=False)])
    lengths[slots] = rng.permutation(LADDER)
    ids, n = ids_with_lengths(lengths, rng)
    return ids, lengths, slots


@functools.lru_cache(maxsize=1)                        # (the cases of one d run one after the other)
def _ladder_case(d):
    ids, lengths, slots = _ladder_ids()
    x = _wide_rows(np.random.default_rng(d), ids.size, d)
    return x, sequential_sums(x, ids, K_LADDER)


def _assert_ladder(ref, lengths, slots, n):
    counts = ref[1]
    assert n <= 64 * K_LADDER                                           # the bucket strategy is eligible
    assert np.array_equal(counts, lengths.astype(np.float32))
    assert sorted(counts[slots].astype(int).tolist()) == sorted(LADDER)
    assert {0, K_LADDER - 1} <= set(slots.tolist())
    assert int((counts > LONG_LIST).sum()) == 17


def _ladder_params():
    out = []
    for d in LADDER_D:
        if d % 4 == 0:
            out += [pytest.param(d, True, 1, id=f"d{d}-buckets"), pytest.param(d, True, 0, id=f"d{d}-sort")]
        else:   # the switch stays at its default: the plan itself must turn to the sort, with every list a short one
            out.append(pytest.param(d, True, 1, id=f"d{d}-sort_forced_by_d%4"))
        if d in (4, 64, 128, 256):
            out.append(pytest.param(d, False, 1, id=f"d{d}-unaligned-sort_forced_by_alignment"))
    return out


@pytest.mark.parametrize("d,aligned,buckets", _ladder_params())
def test_length_ladder(be, switches, d, aligned, buckets):
    """One id vector in which 47 clusters, at shuffled ids including 0 and k - 1, have exactly these member counts:

    short kernel (centroid_accum_kernel): 0, 1, 2, 3 (empty list, first batch); 7, 8, 9 and 15, 16, 17 (RB = 8 / 16:
    `m + RB < cnt`); 31, 32, 33 (`m + 2*RB < cnt` at RB = 16, second round at RB = 8); 63, 64, 65 (the 64-member index
    block, `base + 64 < end`); 79, 80, 81 (64 + RB); 127, 128, 129 and 191, 192, 193 (second / third index block);
    1023, 1024, 1025 (member_sort_kernel's P = next power of two); 2047, 2048 (long_list: the last short list, the
    capacity of member_sort_kernel).
    long kernel (centroid_accum_long_kernel): 2049, 2050 (`> long_list` in the short kernel, bucket_scan_kernel,
    long_detect_kernel and the long kernel at once; one full LONG_CHUNK plus the 1-tail); 4095, 4096, 4097 (two ring
    buffers full); 6143, 6144, 6145 (the first buffer reused); 2 * LONG_CHUNK + {15, 16, 17} (the adder's 16-tail),
    + {127, 128, 129} (its 128-batch), + {143, 144, 145} (128 + 16 + 1).
    That is 17 long clusters: one more than EARLY_MAX, so the sort strategy's second call sums sixteen early and one
    behind the sort, and the bucket strategy rank-sorts one.  Filler clusters of 0 .. 200 rows keep n <= 64 k.
    d selects the plan's width: vec = 1 (d < 128, or odd), vec = 2 (128, 130, 252, 258: 130 and 258 leave one live lane
    in the second slab), vec = 4 (256: one full slab, 260: a second slab with one live lane, 640); unaligned rows and
    d % 4 != 0 make every list a short one (long_list = UINT32_MAX), whatever its length."""
    switches(accum_buckets=buckets)
    ids, lengths, slots = _ladder_ids()
    x, ref = _ladder_case(d)
    _assert_ladder(ref, lengths, slots, ids.size)
    xt = _rows_dev(be, x, aligned)
    for call in range(2):                               # (the sort strategy sums the predicted long clusters early from call 2 on)
        _check(be, x, xt, ids, K_LADDER, f"call {call}", ref=ref)


@pytest.mark.parametrize("d", [8, 64, 256])
def test_long_lists_beyond_the_compaction_are_rank_sorted(be, switches, d):
    """Bucket strategy, 22 long clusters: the sixteen lowest-id ones get their lists from the ordered compaction, the
    six highest -- 2049, 3072, 3073, 4096, 4097, 6144 members: the 1024-wide tiles of long_ranksort_kernel full, one
    over, and the shortest long list -- are scattered, rank-sorted and summed by the second long pass."""
    switches(accum_buckets=1)
    rng = np.random.default_rng(1024 + d)
    k = K_LADDER
    named = [4096, 4097, 6144, 3072, 3073, 2049]
    lengths = rng.integers(0, 201, k) * (rng.random(k) < 0.3)
    low = rng.choice(1500, EARLY_MAX, replace=False)
    lengths[low] = rng.integers(2049, 2700, EARLY_MAX)
    high = np.concatenate([[k - 1], 1500 + rng.choice(k - 1501, len(named) - 1, replace=False)])
    lengths[high] = rng.permutation(named)
    ids, n = ids_with_lengths(lengths, rng)
    assert n <= 64 * k
    x = _wide_rows(rng, n, d)
    ref = sequential_sums(x, ids, k)
    long_ids = np.flatnonzero(ref[1] > LONG_LIST)
    assert long_ids.size == 22 and long_ids.size >= 17
    assert sorted(ref[1][long_ids[EARLY_MAX:]].astype(int).tolist()) == sorted(named)
    assert not set(high.tolist()) & set(long_ids[:EARLY_MAX].tolist())
    xt = _rows_dev(be, x)
    for call in range(2):
        _check(be, x, xt, ids, k, f"call {call}", ref=ref)


# ---- b. sizes -------------------------------------------------------------------------------------------------------
SIZES_N = [0, 1, 2048, 2049, 4096, 4097, 8191, 262144 + 1]


def _size_params():
    out = []
    for n in SIZES_N:
        for layout, k in (("one_cluster", 37), ("one_cluster", 5000), ("spread", 37)):
            if n <= 64 * k:
                out += [pytest.param(n, layout, k, 1, id=f"n{n}-{layout}-k{k}-buckets"),
                        pytest.param(n, layout, k, 0, id=f"n{n}-{layout}-k{k}-sort")]
            else:
                out.append(pytest.param(n, layout, k, 1, id=f"n{n}-{layout}-k{k}-sort_forced_by_n>64k"))
    return out


@pytest.mark.parametrize("n,layout,k,buckets", _size_params())
def test_row_block_edges(be, switches, n, layout, k, buckets):
    """n at the edges of the 4096-row blocks of the ordered compaction (EARLY_ROWS), of rows_per_block of the count /
    scatter passes and of have_long (n = 2049 is the smallest), and n = 0: all rows in one cluster, and spread."""
    switches(accum_buckets=buckets)
    d = 64
    rng = np.random.default_rng(n + k)
    x = _wide_rows(rng, n, d)
    ids = np.full(n, 5, np.int64) if layout == "one_cluster" else rng.integers(0, k, n)
    xt = _rows_dev(be, x)
    for call in range(2):
        _check(be, x, xt, ids, k, f"call {call}")


@pytest.mark.parametrize("n,buckets", [pytest.param(1, 1, id="n1-buckets"), pytest.param(1, 0, id="n1-sort"),
                                       pytest.param(64, 1, id="n64-buckets"), pytest.param(64, 0, id="n64-sort"),
                                       pytest.param(65, 1, id="n65-sort_forced_by_n>64k"),
                                       pytest.param(5000, 1, id="n5000-sort_forced_by_n>64k")])
def test_one_cluster_table(be, switches, n, buckets):
    """k = 1: cluster 0 is also cluster k - 1, every table has two entries, and at n = 5000 the only list is a long one."""
    switches(accum_buckets=buckets)
    rng = np.random.default_rng(n)
    x = _wide_rows(rng, n, 64)
    ids = np.zeros(n, np.int64)
    ids[n // 2] = 1 if n > 2 else 0                     # (one row outside [0, k) where there is room)
    xt = _rows_dev(be, x)
    for call in range(2):
        _check(be, x, xt, ids, 1, f"call {call}")


@functools.lru_cache(maxsize=1)                        # (both strategies at n = 64 k take the same case)
def _largest_table_case(n_extra):
    k, d = 16384, 64
    n = 64 * k + n_extra
    rng = np.random.default_rng(k + n_extra)
    ids = _skewed_ids(rng, n, k, 3, share=0.02)
    x = _wide_rows(rng, n, d)
    return x, ids, sequential_sums(x, ids, k)


@pytest.mark.parametrize("n_extra,buckets", [pytest.param(0, 1, id="n=64k-buckets"), pytest.param(0, 0, id="n=64k-sort"),
                                             pytest.param(1, 1, id="n=64k+1-sort_forced_by_n>64k")])
def test_largest_bucket_table_and_the_strategy_flip(be, switches, n_extra, buckets):
    """k = 16384, the largest table of the bucket strategy and of the count + scan beside the sort (offsets_beside),
    at n = 64 k (the last n the bucket strategy takes) and 64 k + 1; three long lists."""
    switches(accum_buckets=buckets)
    k = 16384
    x, ids, ref = _largest_table_case(n_extra)
    xt = _rows_dev(be, x)
    for call in range(2):
        _check(be, x, xt, ids, k, f"call {call}", ref=ref)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("k,n_long", [(16385, 3), (16385, 20), (20000, 3), (20000, 20)])
def test_tables_past_the_bucket_limit_sort_forced_by_k(be, switches, k, n_long, d):
    """k > 16384: the sort strategy whatever the switch says, with segment_offsets_kernel's binary-searched offsets
    feeding long_detect_kernel and the late long pass (k <= 16384 takes the count + scan beside the sort instead)."""
    switches(accum_buckets=1)
    n = 300000
    rng = np.random.default_rng(k + n_long + d)
    ids = _skewed_ids(rng, n, k, n_long, share=0.5)
    ids[rng.integers(0, n, 30)] = -1
    x = _wide_rows(rng, n, d)
    xt = _rows_dev(be, x)
    ref = sequential_sums(x, ids, k)
    for call in range(2):
        _check(be, x, xt, ids, k, f"call {call}", ref=ref)


# ---- c. id values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buckets", BOTH)
def test_ids_far_outside_the_table_are_parked(be, switches, buckets):
    """-1, INT64_MIN, k, k + 7, 2^31, 2^32 + 0, 2^32 + c for a long cluster c and INT64_MAX all belong to the trailing
    bucket: a cast to 32 bits would make 2^32 + c a member of cluster c (of cluster 0) in the kernels that compare ids
    with the predicted long clusters.  Two calls: in the second c is a predicted cluster of the sort strategy."""
    switches(accum_buckets=buckets)
    d, k = 64, K_LADDER
    base_ids, lengths, slots = _ladder_ids()
    x, base = _ladder_case(d)
    c = int(slots[np.flatnonzero(lengths[slots] == 4097)[0]])
    rng = np.random.default_rng(63)
    ids = base_ids.copy()
    free = np.flatnonzero((ids != c) & (ids != 0))
    values = [-1, -2**63, k, k + 7, 2**31, 2**32, 2**32 + c, 2**63 - 1]
    rows = rng.choice(free, 6 * len(values), replace=False).reshape(len(values), 6)
    for v, r in zip(values, rows):
        ids[r] = v
    ref = sequential_sums(x, ids, k)
    assert int((ref[3] == k).sum()) == rows.size                      # all of them in the trailing bucket
    for cl in (c, 0):                                                 # the aliased clusters: untouched
        assert np.array_equal(bits(ref[0][cl]), bits(base[0][cl])) and ref[1][cl] == base[1][cl]
    xt = _rows_dev(be, x)
    for call in range(2):
        _check(be, x, xt, ids, k, f"call {call}", ref=ref)


# ---- d. row values --------------------------------------------------------------------------------------------------
def _subnormals(rng, shape):
    """|x| around 1e-41: subnormal bit patterns of either sign."""
    b = rng.integers(1, 20000, shape).astype(np.uint32) | (rng.integers(0, 2, shape).astype(np.uint32) << 31)
    return b.view(np.float32)


@pytest.mark.parametrize("buckets", BOTH)
@pytest.mark.parametrize("d", [8, 64, 256])
def test_row_values(be, switches, d, buckets):
    """Per kind a short list (one-wave kernel) and a long one (LDS ring): subnormal rows alone (a denormal flush would
    zero them); normals that cancel pairwise with subnormals in between (a subnormal result); rows of -0.0 (the sum of
    an all -0.0 list is +0.0: it starts from +0.0); +inf and -inf in one cluster (NaN from the second on); a NaN row
    past member 2048 of a long list (NaN from there on, in every feature the row has it); magnitudes over 2^-20 .. 2^20."""
    switches(accum_buckets=buckets)
    k = 600
    rng = np.random.default_rng(d)
    kinds = ["subnormal", "cancel", "negzero", "infs", "nan", "wide"]
    long_len = dict(zip(kinds, [3000, 2500, 2200, 2300, 4200, 2600]))
    short_len = dict(zip(kinds, [70, 33, 10, 20, 50, 100]))
    where = {("long", kd): 10 + 50 * i for i, kd in enumerate(kinds)}
    where.update({("short", kd): 20 + 50 * i for i, kd in enumerate(kinds)})
    sizes = {where[("long", kd)]: long_len[kd] for kd in kinds}
    sizes.update({where[("short", kd)]: short_len[kd] for kd in kinds})
    n = 30000
    assert n <= 64 * k
    ids = _ids_with_long(rng, n, k, sizes)
    x = _wide_rows(rng, n, d, -2, 2)
    for (_, kind), c in where.items():
        rows = np.flatnonzero(ids == c)                               # ascending: the member order
        m = rows.size
        if kind == "subnormal":
            x[rows] = _subnormals(rng, (m, d))
        elif kind == "cancel":
            v = _subnormals(rng, (m, d))                               # triples (a, subnormal, -a) with a around 1e-36:
            first = np.arange(0, m - 2, 3)                            # the subnormal is rounded to a's ulp, then a leaves
            a = (rng.standard_normal((first.size, d)) * 1e-36).astype(np.float32)
            v[first], v[first + 2] = a, -a
            x[rows] = v
        elif kind == "negzero":
            x[rows] = np.float32(-0.0)
        elif kind == "infs":
            x[rows[m // 3], : d // 2] = np.inf
            x[rows[m // 3], d // 2:] = -np.inf
            x[rows[2 * m // 3]] = -np.inf                             # first half: +inf - inf = NaN, second: stays -inf
        elif kind == "nan":
            x[rows[m - 7 if m < 100 else 3000], ::2] = np.nan         # (the long list: in its second ring buffer)
        else:
            x[rows] = _wide_rows(rng, m, d, -20, 20)
    ref = sequential_sums(x, ids, k)
    sums = ref[0]
    for size in ("long", "short"):
        s = sums[where[(size, "subnormal")]]
        assert (np.abs(s) < np.finfo(np.float32).tiny).all() and s.any()
        s = sums[where[(size, "cancel")]]
        assert (np.abs(s) < np.finfo(np.float32).tiny).all() and s.any()
        assert (bits(sums[where[(size, "negzero")]]) == 0).all()
        s = sums[where[(size, "infs")]]
        assert np.isnan(s[: d // 2]).all() and np.isneginf(s[d // 2:]).all()
        s = sums[where[(size, "nan")]]
        assert np.isnan(s[::2]).all() and np.isfinite(s[1::2]).all()
    assert int((ref[1] > LONG_LIST).sum()) == len(kinds)
    xt = _rows_dev(be, x)
    for call in range(2):
        _check(be, x, xt, ids, k, f"call {call}", nan_ok=True, ref=ref)


# ---- e. sequences of calls on one context ---------------------------------------------------------------------------
def test_sequence_k_shrinks_and_grows_back(be, switches):
    """k 3000 -> 500 -> 3000 at one n, sort strategy: WS_LONG_PRED is large enough throughout, so only long_pred_k tells
    that its ids and marks belong to another table; the third call's long clusters include ids >= 500."""
    _known_state(be, switches)
    switches(accum_buckets=0)
    n, d = 100000, 64
    rng = np.random.default_rng(3000)
    x = _wide_rows(rng, n, d)
    xt = _rows_dev(be, x)
    steps = [(3000, {5: 3000, 1200: 2500, 2999: 5000}), (500, {5: 2500, 77: 2100, 499: 4000}),
             (3000, {2: 2600, 700: 3000, 2999: 2049}), (3000, {2: 2600, 700: 3000, 2999: 2049})]
    for i, (k, long) in enumerate(steps):
        _check(be, x, xt, _ids_with_long(rng, n, k, long), k, f"step {i} (k = {k})")


@pytest.mark.parametrize("buckets", BOTH)
def test_sequence_n_grows_and_shrinks_back(be, switches, buckets):
    """n 50 000 -> 400 000 -> 50 000 at one k: the row-sized workspaces are reallocated in the second call, the third
    runs in workspaces larger than it needs, with tables left by a larger call."""
    _known_state(be, switches)
    switches(accum_buckets=buckets)
    k, d = 6400, 64
    rng = np.random.default_rng(6400 + buckets)
    x = _wide_rows(rng, 400000, d)
    xt = _rows_dev(be, x)
    steps = [(50000, {0: 2049, 3000: 4000}), (400000, {0: 30000, 17: 2500, 6399: 9000}), (50000, {17: 2049, 6399: 3000}),
             (50000, {17: 2049, 6399: 3000})]
    for i, (n, long) in enumerate(steps):
        assert n <= 64 * k
        _check(be, x[:n], xt[:n], _ids_with_long(rng, n, k, long), k, f"step {i} (n = {n})")


def test_sequence_strategy_alternates(be, switches):
    """accum_buckets 1 -> 0 -> 1 -> 0 at one (n, k): the bucket strategy's counters and the sort strategy's count + scan
    beside the sort (offsets_beside) share WS_BUCKETS, whose counters must be zero between calls whoever ran last."""
    _known_state(be, switches)
    n, k, d = 100000, 2000, 64
    rng = np.random.default_rng(2000)
    x = _wide_rows(rng, n, d)
    xt = _rows_dev(be, x)
    for i, b in enumerate([1, 0, 1, 0, 0, 1]):
        switches(accum_buckets=b)
        long = {int(c): int(m) for c, m in zip(rng.choice(k, 4, replace=False), rng.integers(2049, 6000, 4))}
        _check(be, x, xt, _ids_with_long(rng, n, k, long), k, f"step {i} (accum_buckets = {b})")


def test_sequence_stale_predictions(be, switches):
    """Sort strategy, one k: every call's early pass works from the long clusters of the call before, which are wrong in
    a different way each time."""
    _known_state(be, switches)
    switches(accum_buckets=0)
    n, k, d = 80000, 2000, 64
    rng = np.random.default_rng(80000)
    x = _wide_rows(rng, n, d)
    xt = _rows_dev(be, x)
    many = {0: 2300}
    many.update({int(c): 2100 + 10 * j for j, c in enumerate(1 + rng.choice(k - 1, 19, replace=False))})
    steps = [("first", n, {10: 3000, 20: 2500, 30: 4097}, ()),
             ("long set disjoint from the last", n, {11: 3000, 21: 2500, 31: 4097}, ()),
             ("every predicted cluster empty", n, {40: 5000, 41: 2600}, (11, 21, 31)),
             ("a predicted cluster at 2048, another at 2049", n, {40: 2048, 41: 2049}, ()),
             ("all ids invalid", n, None, ()),
             ("no rows", 0, None, ()),
             ("normal again", n, {10: 2500, 41: 3000}, ()),
             ("twenty long, cluster 0 among them", n, many, ()),
             ("two long, cluster 0 among them", n, {0: 2600, k - 1: 2049}, ())]
    for i, (what, m, long, empty) in enumerate(steps):
        ids = np.full(m, -1, np.int64) if long is None else _ids_with_long(rng, m, k, long, empty)
        ref = _check(be, x[:m], xt[:m], ids, k, f"step {i} ({what})")
        if long:
            assert set(np.flatnonzero(ref[1] > LONG_LIST).tolist()) == {c for c, v in long.items() if v > LONG_LIST}


def test_sequence_drifting_long_set_over_forty_calls(be, switches):
    """40 calls at one k, sort strategy, long_gen advancing: four long clusters that wander back and forth over
    neighbouring ids, so a cluster that was summed early (and marked) some calls ago is long again in a call that did
    not predict it -- the pass behind the sort must take it, whatever its old mark says."""
    _known_state(be, switches)
    switches(accum_buckets=0)
    n, k, d = 40000, 1000, 8
    rng = np.random.default_rng(40)
    x = _wide_rows(rng, n, d)
    xt = _rows_dev(be, x)
    base, wander = [5, 300, 600, 985], [0, 1, 2, 1]
    for t in range(40):
        long = {base[j] + wander[((t + j) // 2) % 4]: int(rng.integers(2049, 3500)) for j in range(4)}
        _check(be, x, xt, _ids_with_long(rng, n, k, long), k, f"call {t}", want_order=(t % 5 == 0))


def test_sequence_marks_do_not_share_a_word_with_the_predicted_ids(be, switches):
    """WS_LONG_PRED keeps [count | EARLY_MAX predicted ids | k generation marks] (LongPred::MARKS_AT).  Were the marks
    laid over the last predicted id, whatever long_detect_kernel writes there would be cluster 0's mark, and cluster 0
    is left un-summed in the call whose generation equals it.  Sort strategy, generations counted from a known state.
    Call 1 has exactly EARLY_MAX long clusters, with ids 2, 4, .. 32: whichever of them takes the last slot (the slots
    go in the order the lanes' atomics arrive, which nothing fixes), it stays there, since no later call has as many.
    Cluster 0 is long in every even call from 2 to 32 and short in between, so it is never long in a call that predicted
    it (the odd call's early pass leaves a short list before the mark) and is never marked: each even call takes it
    behind the sort, unless its "mark" says the call's own generation."""
    _known_state(be, switches)
    switches(accum_buckets=0)
    n, k, d = 70000, 1000, 8
    rng = np.random.default_rng(16)
    x = _wide_rows(rng, n, d)
    xt = _rows_dev(be, x)
    last_slot = list(range(2, 2 * EARLY_MAX + 1, 2))
    for g in range(1, 2 * EARLY_MAX + 2):               # (the g-th call with this k takes generation g)
        if g == 1:
            long = {c: 2049 + int(rng.integers(0, 300)) for c in last_slot}
        else:
            long = {500: 2100, 600 + g: 2200}
            if g in last_slot:
                long[0] = 2500
        ref = _check(be, x, xt, _ids_with_long(rng, n, k, long), k, f"call {g}", want_order=False)
        assert sorted(np.flatnonzero(ref[1] > LONG_LIST).tolist()) == sorted(long)


@pytest.mark.parametrize("buckets", BOTH)
def test_sequence_want_order_alternates(be, switches, buckets):
    """want_order True / False in turn: the bucket strategy joins the side stream before the order leaves the workspace
    (the long clusters' segments are written there), the sort strategy copies it out of the sort's buffers."""
    _known_state(be, switches)
    switches(accum_buckets=buckets)
    n, k, d = 90000, 1500, 64
    rng = np.random.default_rng(1500 + buckets)
    x = _wide_rows(rng, n, d)
    xt = _rows_dev(be, x)
    for i, want in enumerate([True, False, True, False, True, True]):
        long = {int(c): int(m) for c, m in zip(rng.choice(k, 18 if i == 4 else 3, replace=False), rng.integers(2049, 4000, 18))}
        _check(be, x, xt, _ids_with_long(rng, n, k, long), k, f"step {i} (want_order = {want})", want_order=want)


@pytest.mark.parametrize("buckets", BOTH)
def test_sequence_deferred_join_and_another_stream(be, switches, buckets):
    """defer_join=True, independent work behind it, centroid_accum_join(), then the result; the same on a stream that
    is not the default one; then a plain call on the default stream."""
    _known_state(be, switches)
    switches(accum_buckets=buckets)
    n, k, d = 90000, 1500, 64
    rng = np.random.default_rng(77 + buckets)
    x = _wide_rows(rng, n, d)
    xt = _rows_dev(be, x)
    cases = []
    for i in range(3):
        ids = _ids_with_long(rng, n, k, {3 + i: 30000, 700: 2049 + i, k - 1: 4096})
        cases.append((ids, _ids_dev(be, ids), sequential_sums(x, ids, k), _out(be, k, d)))   # (alive to the end)
    ids, idt, ref, out = cases[0]
    part = be.centroid_accum(xt, idt, k, out=out, defer_join=True)
    busy = be.l2norm_rows(xt)                            # needs nothing of the sums
    be.centroid_accum_join()
    _verify(be, part, ref, k, d, want_order=False, label="deferred, default stream")
    s = torch.cuda.Stream(device=be.device)
    s.wait_stream(torch.cuda.current_stream(be.device))
    ids, idt, ref, out = cases[1]
    with torch.cuda.stream(s):
        part = be.centroid_accum(xt, idt, k, out=out, defer_join=True)
        busy2 = be.l2norm_rows(xt)
        be.centroid_accum_join()
        _verify(be, part, ref, k, d, want_order=False, label="deferred, another stream")
        got = be.centroid_accum(xt, idt, k, out=_out(be, k, d), want_order=True)
        _verify(be, got, ref, k, d, label="joined, another stream")
    s.synchronize()
    ids, idt, ref, out = cases[2]
    got = be.centroid_accum(xt, idt, k, out=out, want_order=True)
    _verify(be, got, ref, k, d, label="plain call afterwards")
    assert torch.equal(busy, busy2)


@pytest.mark.parametrize("buckets", BOTH)
def test_sequence_back_to_back_calls_read_afterwards(be, switches, buckets):
    """Two calls with different ids and result buffers, nothing read in between: the second call's side-stream work
    must not touch the shared workspaces before the first call's kernels have read them."""
    _known_state(be, switches)
    switches(accum_buckets=buckets)
    n, k, d = 200000, 4000, 64
    rng = np.random.default_rng(4000 + buckets)
    x = _wide_rows(rng, n, d)
    xt = _rows_dev(be, x)
    ids_a = _ids_with_long(rng, n, k, {1: 40000, 2000: 2049, k - 1: 9000})
    ids_b = _ids_with_long(rng, n, k, {1: 2049, 7: 50000, 3000: 4097})
    ta, tb = _ids_dev(be, ids_a), _ids_dev(be, ids_b)
    outs = [_out(be, k, d) for _ in range(4)]
    got = [be.centroid_accum(xt, t, k, out=o, want_order=True) for t, o in zip((ta, tb, ta, tb), outs)]
    ref_a, ref_b = sequential_sums(x, ids_a, k), sequential_sums(x, ids_b, k)
    for i, (g, r) in enumerate(zip(got, (ref_a, ref_b, ref_a, ref_b))):
        _verify(be, g, r, k, d, label=f"call {i}")


# ---- f. partial results of several ranks ----------------------------------------------------------------------------
@pytest.mark.parametrize("buckets", BOTH)
@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_partials_of_contiguous_shards(be, switches, P, buckets):
    """The ladder's rows cut into P contiguous ranges, as the ranks hold them; every shard accumulated into its row of a
    stack of packed partials that carry the objective slot behind the counts (row stride != k d + k); then
    centroid_finalize and sum_parts over the stack against the part-ordered fp32 sums."""
    switches(accum_buckets=buckets)
    d, k = 64, K_LADDER
    ids, lengths, slots = _ladder_ids()
    x, _ = _ladder_case(d)
    off, total = be.part_layout(k, d)
    assert total != k * d + k
    parts = torch.full((P, total), float("nan"), dtype=torch.float32, device=be.device)
    cuts = np.linspace(0, ids.size, P + 1).astype(int)
    refs = []
    for p in range(P):
        lo, hi = cuts[p], cuts[p + 1]
        assert hi - lo <= 64 * k
        refs.append(sequential_sums(x[lo:hi], ids[lo:hi], k))
        got = be.centroid_accum(_rows_dev(be, x[lo:hi]), _ids_dev(be, ids[lo:hi]), k, out=parts[p], want_order=True)
        _verify(be, got, refs[p], k, d, label=f"shard {p} of {P}")
    parts[:, off:] = 3.0                                              # the objective slot: any finite bits
    shard_counts = np.stack([r[1] for r in refs])
    assert (shard_counts.sum(0) == 0).any()                           # a cluster empty in every shard
    if P > 1:
        assert ((shard_counts == 0).any(0) & (shard_counts.sum(0) > 0)).any()   # and one empty in some shards only
    r_cent, r_h = finalize(np.stack([r[0] for r in refs]), shard_counts)
    cent, h = be.centroid_finalize(parts, k, d)
    _same(cent.cpu().numpy(), r_cent, False, "finalize over the stack")
    _same(h.cpu().numpy(), r_h, False, "hassign over the stack")
    assert np.array_equal(r_h, lengths.astype(np.float32))
    host = parts.cpu().numpy()
    _same(be.sum_parts(parts).cpu().numpy(), sum_parts(host), False, "sum_parts")
