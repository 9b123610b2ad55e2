"""CPU reference of the MFCC / delta features (ops.MFCC, ops.ComputeDeltas, at_mfcc_f32, at_deltas_f32), numpy float32
only.  TEST ONLY.

The contract: per clip, the optional top_db clamp at the clip's own maximum; coefficients by the
fp32 fmaf chain over the mel index, ascending, from +0; deltas by the regression chain acc = fmaf(j, c[t + j] - c[t - j],
acc) for j = 1 .. N with the neighbours clamped to the frame's own clip, then one division by (float)(N (N + 1) (2N + 1)
/ 3); the second order is the same operator on the first.  fma32 (spherical_ref) is an exact fmaf; subtraction and
division are numpy's own float32 operations.  No float64 in the value path; the DCT table is an input (its own
definition, in double by contract, is dct_table below)."""
import numpy as np

from spherical_ref import fma32

TB = 64    # frames per workgroup of the kernel at every width the tests of the tile edges use (csrc/mfcc.hip)


def dct_table(n_mfcc, n_mels, ortho=True):
    """at_dct_matrix_host restated: [n_mels, n_mfcc] float32."""
    n = np.arange(n_mels, dtype=np.float64)[:, None]
    k = np.arange(n_mfcc, dtype=np.float64)[None, :]
    t = np.cos(np.pi / n_mels * (n + 0.5) * k)
    if ortho:
        t[:, 0] *= 1.0 / np.sqrt(2.0)
        t *= np.sqrt(2.0 / n_mels)
    else:
        t *= 2.0
    return t.astype(np.float32)


def prefix_of(counts):
    counts = np.asarray(counts, dtype=np.int64)
    first = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=first[1:])
    return first


def clip_bounds(counts):
    """-> (start, end) int64 [n]: the clip of every global frame."""
    counts = np.asarray(counts, dtype=np.int64)
    first = prefix_of(counts)
    return np.repeat(first[:-1], counts), np.repeat(first[1:], counts)


def top_db_ref(x, counts, top_db):
    x = np.array(x, dtype=np.float32)
    first = prefix_of(counts)
    for i in range(len(counts)):
        v = x[first[i]:first[i + 1]]
        if v.size == 0:
            continue
        if np.isnan(v).any():
            v[...] = np.nan
            continue
        with np.errstate(invalid="ignore"):
            floor = np.float32(v.max()) - np.float32(top_db)
            v[...] = np.where(v < floor, floor, v)
    return x


def coefficients_ref(x, dct):
    x = np.ascontiguousarray(x, dtype=np.float32)
    dct = np.ascontiguousarray(dct, dtype=np.float32)
    acc = np.zeros((x.shape[0], dct.shape[1]), np.float32)
    for n in range(x.shape[1]):
        acc = fma32(x[:, n:n + 1], dct[n][None, :], acc)
    return acc


def deltas_ref(c, counts, win_length):
    """c [n, F] float32 -> [n, F]: the delta operator over the frames of every clip."""
    c = np.ascontiguousarray(c, dtype=np.float32)
    assert win_length >= 3 and win_length % 2 == 1
    N = (win_length - 1) // 2
    denom = np.float32(N * (N + 1) * (2 * N + 1) // 3)
    s, e = clip_bounds(counts)
    g = np.arange(c.shape[0], dtype=np.int64)
    acc = np.zeros_like(c)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(1, N + 1):
            diff = c[np.minimum(g + j, e - 1)] - c[np.maximum(g - j, s)]
            assert diff.dtype == np.float32
            acc = fma32(np.float32(j), diff, acc)
        out = acc / denom
    assert out.dtype == np.float32
    return out


def mfcc_ref(x, counts, dct, orders=0, win_length=5, top_db=None):
    """-> [n, n_mfcc * (1 + orders)] float32, frame-major."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert sum(counts) == x.shape[0]
    if top_db is not None:
        x = top_db_ref(x, counts, top_db)
    parts = [coefficients_ref(x, dct)]
    for _ in range(orders):
        parts.append(deltas_ref(parts[-1], counts, win_length))
    return np.concatenate(parts, axis=1)


def feature_major(out, counts):
    """frame-major [n, D] -> the flat feature-major form: clip i a [D, T_i] block at D * first_frame[i]."""
    first = prefix_of(counts)
    return np.concatenate([out[first[i]:first[i + 1]].T.reshape(-1) for i in range(len(counts))] +
                          [np.zeros(0, np.float32)])


def same_bits(got, ref):
    """Equal bit for bit, NaN positions equal (a NaN's payload is not part of the contract)."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != np.float32 or ref.dtype != np.float32:
        return False
    gn, rn = np.isnan(got), np.isnan(ref)
    return bool(np.array_equal(gn, rn) and np.array_equal(got.view(np.uint32)[~gn], ref.view(np.uint32)[~rn]))


# ---- the torchaudio composition, restated (torchaudio is not installed), and the data-derived bounds of the tests ----

U = 2.0 ** -24


def gamma(m):
    return m * U / (1 - m * U)


def create_dct_torch(n_mfcc, n_mels, norm="ortho"):
    """torchaudio.functional.create_dct: the cosine evaluated in float32 -> torch float32 [n_mels, n_mfcc]."""
    import math

    import torch
    n = torch.arange(float(n_mels))
    k = torch.arange(float(n_mfcc)).unsqueeze(1)
    dct = torch.cos(math.pi / float(n_mels) * (n + 0.5) * k)
    if norm is None:
        dct *= 2.0
    else:
        dct[0] *= 1.0 / math.sqrt(2.0)
        dct *= math.sqrt(2.0 / float(n_mels))
    return dct.t().contiguous()


def compute_deltas_torch(specgram, win_length=5):
    """torchaudio.functional.compute_deltas(specgram [..., F, T], win_length, mode="replicate")."""
    import torch
    shape = specgram.size()
    specgram = specgram.reshape(1, -1, shape[-1])
    n = (win_length - 1) // 2
    denom = n * (n + 1) * (2 * n + 1) / 3
    specgram = torch.nn.functional.pad(specgram, (n, n), mode="replicate")
    kernel = torch.arange(-n, n + 1, 1, dtype=specgram.dtype).repeat(specgram.shape[1], 1, 1)
    return (torch.nn.functional.conv1d(specgram, kernel, groups=specgram.shape[1]) / denom).reshape(shape)


def amplitude_to_db_clamp_torch(x_db, top_db):
    """The last step of torchaudio.functional.amplitude_to_DB on one clip passed alone: x_db [F, T] already in dB."""
    import torch
    return torch.max(x_db, (x_db.amax() - top_db))


def delta_exact_and_bound(v, b, counts, win_length, steps):
    """v [n, F] float64: exact values; b [n, F]: |computed - v| <= b.  -> (dv, db): the exact deltas of v, and a bound
    of |computed delta - dv| for a computation that takes the computed values, forms the weighted sum in at most
    `steps` float32 roundings per term (Higham, section 3.1: gamma_steps * sum |terms|) and divides once."""
    N = (win_length - 1) // 2
    denom = N * (N + 1) * (2 * N + 1) / 3
    s, e = clip_bounds(counts)
    g = np.arange(v.shape[0], dtype=np.int64)
    dv, mag, carried = np.zeros_like(v), np.zeros_like(v), np.zeros_like(v)
    for j in range(1, N + 1):
        ip, im = np.minimum(g + j, e - 1), np.maximum(g - j, s)
        dv += j * (v[ip] - v[im])
        mag += j * (np.abs(v[ip]) + b[ip] + np.abs(v[im]) + b[im])
        carried += j * (b[ip] + b[im])
    return dv / denom, (carried + gamma(steps) * mag) / denom
