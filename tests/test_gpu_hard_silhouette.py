"""at_silhouette_f32 on the hard data of tests/hard_silhouette_data.py, on the MI355X, bit for bit against
tests/silhouette_ref.py: on grid rows and in one dimension the recipe leaves no freedom (see the data module), so every
row of every such rung has to carry the reference's bits, nothing exempt.  tests/test_hard_silhouette_ref.py proves
that the rungs are what their names say."""
import functools

import numpy as np
import pytest
import torch

import hard_silhouette_data as hs
from silhouette_ref import silhouette_samples_ref
from test_gpu_silhouette import S_TOL, SCORE_TOL

pytestmark = pytest.mark.gpu

LARGE = "seams-65-1025-planted"
SMALL = "seams-3-33-planted"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _ref(name):
    x, lab = hs.rung(name)
    with np.errstate(all="ignore"):
        s = silhouette_samples_ref(x, lab)
    s.setflags(write=False)
    return s


def _dev(be, name):
    """The rung on the device (from copies: the shared host arrays are read-only)."""
    x, lab = hs.rung(name)
    return be.from_host(x.copy()), be.from_host(lab.copy())


def _same_bits(got, name, what=""):
    ref = _ref(name)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (name, what, got.dtype, got.shape)
    wrong = np.flatnonzero(bits(got) != bits(ref))
    assert wrong.size == 0, (name, what, len(wrong), wrong[:6], got[wrong[:6]], ref[wrong[:6]], bits(got)[wrong[:6]],
                             bits(ref)[wrong[:6]])


@pytest.mark.parametrize("name", hs.BITWISE)
def test_bit_for_bit(be, name):
    x, lab = _dev(be, name)
    total = be.empty((1,), torch.float64)
    s = be.to_host(be.silhouette_samples(x, lab, sum_out=total))
    _same_bits(s, name)
    ref = _ref(name)
    assert abs(float(total.item()) / len(ref) - float(ref.astype(np.float64).sum() / len(ref))) <= SCORE_TOL


def test_label_counts_are_still_refused(be):
    x, lab = _dev(be, SMALL)
    with pytest.raises(ValueError, match="Number of labels is 1. Valid values are 2 to n_samples - 1"):
        be.silhouette_samples(x, np.full(len(x), hs.I64_MIN))
    with pytest.raises(ValueError, match="Number of labels is 33. Valid values are 2 to n_samples - 1"):
        be.silhouette_samples(x, np.arange(len(x)) * 2 ** 40 + hs.I64_MIN)
    _same_bits(be.to_host(be.silhouette_samples(x, lab)), SMALL, "after the refusals")


def test_cancel_within_the_projects_tolerance(be):
    x, lab = _dev(be, "cancel")
    ref = _ref("cancel")
    total = be.empty((1,), torch.float64)
    s = be.to_host(be.silhouette_samples(x, lab, sum_out=total))
    print("cancel: %.4f of the rows bit-equal, largest difference %.3g"
          % (float((bits(s) == bits(ref)).mean()), float(np.abs(s.astype(np.float64) - ref).max())))
    assert np.abs(s.astype(np.float64) - ref).max() <= S_TOL
    assert abs(float(total.item()) / len(ref) - float(ref.astype(np.float64).mean())) <= SCORE_TOL


def test_call_order_leaves_nothing_in_the_workspace(be):
    """A large sample, a small one, the large one again, a wide one, a one-dimensional one: offsets, segments, norms
    and the staged slabs of the call before must not show."""
    for step, name in enumerate([LARGE, SMALL, LARGE, "grid_d-0-200", "grid_d-1048576-1", SMALL, "order-mixed", "tiny76",
                                 LARGE]):
        x, lab = _dev(be, name)
        _same_bits(be.to_host(be.silhouette_samples(x, lab)), name, "step %d" % step)


@pytest.mark.parametrize("name", ["grid_d-1048576-65", "seams-65-513-planted", "grid_d-0-127"])
def test_rows_and_labels_at_offset_pointers(be, name):
    x, lab = hs.rung(name)
    n, d = x.shape
    assert d % 2 == 1
    big = torch.full((n + 1, d), 3.0e38, device=be.device)
    big[1:].copy_(torch.from_numpy(x.copy()))
    big_lab = torch.full((n + 1,), 77, dtype=torch.int64, device=be.device)
    big_lab[1:].copy_(torch.from_numpy(lab.copy()))
    xv, lv = big[1:], big_lab[1:]
    assert xv.is_contiguous() and xv.data_ptr() % 8 == 4 and lv.data_ptr() % 16 == 8
    _same_bits(be.to_host(be.silhouette_samples(xv, lv)), name, "offset")
    _same_bits(be.to_host(be.silhouette_samples(xv.clone(), lv.clone())), name, "fresh copy")


def test_on_a_second_stream(be):
    xd, ld = _dev(be, LARGE)
    xsd, lsd = _dev(be, SMALL)
    _same_bits(be.to_host(be.silhouette_samples(xd, ld)), LARGE, "first stream")
    side = torch.cuda.Stream(device=be.device)
    side.wait_stream(torch.cuda.current_stream(be.device))
    with torch.cuda.stream(side):
        small = be.silhouette_samples(xsd, lsd)                  # the slot changes hands with other sizes in it
        got = be.silhouette_samples(xd, ld)
        got_host, small_host = be.to_host(got), be.to_host(small)
    side.synchronize()
    _same_bits(got_host, LARGE, "side stream")
    _same_bits(small_host, SMALL, "side stream")
    _same_bits(be.to_host(be.silhouette_samples(xd, ld)), LARGE, "back on the first stream")


@pytest.mark.parametrize("name", ["order-ones_first", "order-mixed", "tiny70", "tiny76"])
def test_two_calls_give_the_same_bits(be, name):
    xd, ld = _dev(be, name)
    t1, t2 = be.empty((1,), torch.float64), be.empty((1,), torch.float64)
    s1 = be.silhouette_samples(xd, ld, sum_out=t1).clone()
    s2 = be.silhouette_samples(xd, ld, sum_out=t2)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert t1.item() == t2.item()
    _same_bits(be.to_host(s2), name)
