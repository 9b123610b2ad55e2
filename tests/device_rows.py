"""Rows placed on the device at a chosen alignment, for the tests of the kernels' `at_aligned16` branches."""
import torch


def rows_one_float_off(x, device):
    """The numpy rows x[n, d] on `device` as a contiguous view that starts one float behind a 16-byte boundary."""
    n, d = x.shape
    base = torch.empty(n * d + 1, dtype=torch.float32, device=device)
    base[1:].copy_(torch.from_numpy(x).reshape(-1))
    t = base[1:].view(n, d)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t
