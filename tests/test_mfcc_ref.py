"""tests/mfcc_ref.py, the CPU model of DESIGN.md section 6k, held to independent code (no GPU): the library's DCT
table against scipy's transform of the identity, the coefficient chain against scipy's transform of the float64 input,
the delta chain against torch's padded grouped conv1d (torchaudio's compute_deltas restated), each within a bound computed
from the data; and the argument errors of ops.MFCC, ops.ComputeDeltas and AudioTokenizer.from_features."""
import ctypes

import numpy as np
import pytest
import scipy.fft
import torch

import mfcc_ref as R
from oracle_backend import OracleBackend

SHAPES = [(64, 13), (64, 40), (64, 64), (128, 40), (40, 40), (23, 13), (64, 1)]


def lib_table(n_mfcc, n_mels, ortho=1):
    from audio_tokens_amd import _lib
    out = np.full((n_mels, n_mfcc), np.nan, np.float32)
    assert _lib.load().at_dct_matrix_host(n_mfcc, n_mels, ortho, ctypes.c_void_p(out.ctypes.data)) == 0
    return out


def scipy_table(n_mfcc, n_mels, norm="ortho"):
    return scipy.fft.dct(np.eye(n_mels), type=2, norm=norm, axis=1)[:, :n_mfcc]


@pytest.mark.parametrize("n_mels,n_mfcc", SHAPES)
@pytest.mark.parametrize("norm", ["ortho", None])
def test_table_is_the_correctly_rounded_dct(n_mels, n_mfcc, norm):
    """Half an fp32 ulp of each entry, plus 1e-13: what a double evaluation of cos at an argument of up to 400 rad that
    carries three roundings (400 * 3 * 2^-53 = 1.3e-13) can be off by, which decides the rounding only at a tie."""
    t = lib_table(n_mfcc, n_mels, 1 if norm == "ortho" else 0)
    s = scipy_table(n_mfcc, n_mels, norm)
    tol = 0.5 * np.spacing(np.abs(s).astype(np.float32)).astype(np.float64) + 1e-13
    err = np.abs(t.astype(np.float64) - s)
    assert (err <= tol).all(), float((err / tol).max())
    assert np.array_equal(t.view(np.uint32), R.dct_table(n_mfcc, n_mels, norm == "ortho").view(np.uint32))


def test_table_argument_errors():
    from audio_tokens_amd import _lib
    lib = _lib.load()
    out = np.zeros((4, 4), np.float32)
    p = ctypes.c_void_p(out.ctypes.data)
    for args in [(0, 4, 1, p), (5, 4, 1, p), (4, 0, 1, p), (4, 4, 1, None)]:
        assert lib.at_dct_matrix_host(*args) == -1 and b"at_dct_matrix_host" in lib.at_last_error()


def test_torch_float32_table_is_the_less_accurate_one():
    """The stated deviation: create_dct evaluates the cosine in float32."""
    for n_mels, n_mfcc in [(40, 40), (64, 40)]:
        s = scipy_table(n_mfcc, n_mels)
        ours = np.abs(lib_table(n_mfcc, n_mels).astype(np.float64) - s).max()
        theirs = np.abs(R.create_dct_torch(n_mfcc, n_mels).numpy().astype(np.float64) - s).max()
        assert ours < 3e-8 and 1e-7 < theirs < 1e-5, (ours, theirs)


def _rows(n, n_mels, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, n_mels)) * 18 - 35).astype(np.float32)     # dB-like


@pytest.mark.parametrize("n_mels,n_mfcc", SHAPES)
def test_coefficients_against_scipy(n_mels, n_mfcc):
    x = _rows(97, n_mels, n_mels * 100 + n_mfcc)
    t = lib_table(n_mfcc, n_mels)
    got = R.coefficients_ref(x, t).astype(np.float64)
    want = scipy.fft.dct(x.astype(np.float64), type=2, norm="ortho", axis=1)[:, :n_mfcc]
    ax = np.abs(x.astype(np.float64))
    bound = R.gamma(n_mels) * (ax @ np.abs(t.astype(np.float64))) \
        + ax @ np.abs(t.astype(np.float64) - scipy_table(n_mfcc, n_mels)) + 1e-12
    err = np.abs(got - want)
    assert (err <= bound).all(), float((err / bound).max())
    assert err.max() > 0      # (the bound is not vacuous: the chain does round)


@pytest.mark.parametrize("win_length", [3, 5, 9])
@pytest.mark.parametrize("F", [1, 13, 64])
def test_deltas_against_the_padded_grouped_conv(win_length, F):
    N = (win_length - 1) // 2
    counts = [1, 2, 3, 0, 2 * N, 2 * N + 1, 4 * N + 1, 0, 0, 70]
    c = _rows(sum(counts), F, 7 * win_length + F)
    got = R.deltas_ref(c, counts, win_length).astype(np.float64)
    first = R.prefix_of(counts)
    want = np.concatenate([R.compute_deltas_torch(torch.from_numpy(c[first[i]:first[i + 1]].T.copy()), win_length).numpy().T
                           for i in range(len(counts)) if counts[i]])
    v = c.astype(np.float64)
    exact, b_ours = R.delta_exact_and_bound(v, np.zeros_like(v), counts, win_length, N + 2)
    _, b_torch = R.delta_exact_and_bound(v, np.zeros_like(v), counts, win_length, 2 * N + 2)
    assert (np.abs(got - exact) <= b_ours + 1e-300).all()
    assert (np.abs(got - want) <= b_ours + b_torch + 1e-300).all()


def test_model_edges():
    t = lib_table(13, 23)
    counts = [5, 1, 0, 9]
    x = _rows(15, 23, 3)
    x[:5] = x[0]                                                 # a constant clip
    out = R.mfcc_ref(x, counts, t, orders=2, win_length=5)
    assert out.shape == (15, 39)
    assert not out[:6, 13:].view(np.uint32).any()                # constant clip and T = 1: exactly +0
    assert out[6:, 13:].view(np.uint32).any()
    fm = R.feature_major(out, counts)
    assert np.array_equal(fm[:39 * 5].reshape(39, 5), out[:5].T) and np.array_equal(fm[39 * 6:].reshape(39, 9), out[6:].T)
    # top_db: per clip; a NaN takes its clip and no other
    x[8, 3] = np.nan
    y = R.top_db_ref(x, counts, 20.0)
    assert np.isnan(y[6:]).all() and not np.isnan(y[:6]).any()
    assert y[:5].min() >= x[:5].max() - np.float32(20.0)
    # the reach of a bad frame: orders * N frames on either side, inside the clip
    x = _rows(40, 23, 4)
    x[20, 0] = np.nan
    out = R.mfcc_ref(x, [10, 30], t, orders=2, win_length=5)
    bad = np.isnan(out).any(axis=1)
    assert bad[16:25].all() and not bad[:16].any() and not bad[25:].any()
    assert R.same_bits(out, out.copy()) and not R.same_bits(out, np.nan_to_num(out))


def test_ops_argument_errors():
    from audio_tokens_amd import ops
    be = OracleBackend()
    with pytest.raises(ValueError):
        ops.MFCC(dct_type=3, backend=be)
    with pytest.raises(NotImplementedError):
        ops.MFCC(log_mels=True, backend=be)
    with pytest.raises(ValueError):
        ops.MFCC(n_mfcc=65, n_mels=64, backend=be)
    with pytest.raises(ValueError):
        ops.MFCC(n_mfcc=0, backend=be)
    with pytest.raises(ValueError):
        ops.MFCC(deltas=3, backend=be)
    with pytest.raises(ValueError):
        ops.MFCC(win_length=4, backend=be)
    with pytest.raises(ValueError):
        ops.MFCC(win_length=1, backend=be)
    with pytest.raises(ValueError):
        ops.MFCC(top_db=-1.0, backend=be)
    with pytest.raises(ValueError):
        ops.MFCC(norm="forward", backend=be)
    with pytest.raises(ValueError):
        ops.MFCC(dct=np.zeros((40, 64), np.float32), backend=be)
    with pytest.raises(ValueError):
        ops.ComputeDeltas(mode="constant", backend=be)
    with pytest.raises(ValueError):
        ops.ComputeDeltas(win_length=6, backend=be)
    m = ops.MFCC(n_mfcc=13, deltas=2, top_db=None, norm=None, backend=be)
    assert m.D == 39 and m.to("cuda") is m and ops.ComputeDeltas(backend=be).win_length == 5
    assert np.array_equal(be.dct_matrix(13, 64, None), lib_table(13, 64, 0))


def test_audio_tokenizer_rejects_features_with_conv():
    """The feature path is AudioTokenizer.from_features (the constructor's own argument list is pinned by
    test_audio_tokens_abi.py); conv beside it, and anything but an ops.MFCC, raise ValueError before any work."""
    from audio_tokens_amd import ops
    be = OracleBackend()
    feats = ops.MFCC(n_mfcc=13, deltas=2, backend=be)
    vocab = np.zeros((8, 39), np.float32)
    with pytest.raises(ValueError):
        ops.AudioTokenizer.from_features(vocab, feats, conv=torch.nn.Conv1d(1, 2, 3, padding=1), backend=be)
    with pytest.raises(ValueError):
        ops.AudioTokenizer.from_features(vocab, "mfcc", backend=be)
