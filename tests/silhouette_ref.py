"""Chunked numpy copy of sklearn's float32 silhouette recipe (include/audio_tokens_amd.h, at_silhouette_f32), in fp64.

Steps: labels as after a LabelEncoder; d2 = fl32(((-2 <x_i,x_j>) + |x_i|^2) + |x_j|^2) with the dot and the norms in
fp64, clamped at 0, 0 for i == j, fp32 square root; S[i,c] = fl32(fp64 sum of the distances to the members of c, in
ascending j); a = fl32(S[i,own] / (n_own - 1)); b = min over c != own of fl32(S[i,c] / n_c);
s = fl32(fl32(b - a) / max(a, b)), NaN -> 0; score = fp64 sum of s / n."""
from __future__ import annotations

import numpy as np


def check_labels(labels, n):
    _, enc = np.unique(np.asarray(labels).reshape(-1), return_inverse=True)
    k = int(enc.max()) + 1 if enc.size else 0
    if not 2 <= k <= n - 1:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % k)
    return enc.astype(np.int64), k


def silhouette_samples_ref(X, labels, chunk=512):
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0]
    enc, k = check_labels(labels, n)
    freq = np.bincount(enc, minlength=k)
    X64 = X.astype(np.float64)
    nrm = np.einsum("ij,ij->i", X64, X64)
    s = np.empty(n, np.float32)
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        d2 = ((-2.0 * (X64[i0:i1] @ X64.T)) + nrm[i0:i1, None]) + nrm[None, :]
        d2 = np.maximum(d2.astype(np.float32), np.float32(0))
        rows = np.arange(i1 - i0)
        d2[rows, rows + i0] = 0
        dist = np.sqrt(d2)                                   # fp32, correctly rounded
        S = np.zeros((i1 - i0, k), np.float32)
        for r in range(i1 - i0):                             # np.bincount: fp64, ascending j
            S[r] += np.bincount(enc, weights=dist[r], minlength=k)
        own = enc[i0:i1]
        a_sum = S[rows, own].copy()
        S[rows, own] = np.inf
        S /= freq                                            # fl32(f64(S) / n_c)
        b = S.min(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            a_sum /= (freq - 1).take(own)                    # fl32(f64(S_own) / (n_own - 1)); 0 / 0 = NaN
            si = (b - a_sum) / np.maximum(a_sum, b)
        s[i0:i1] = np.nan_to_num(si)
    return s


def silhouette_score_ref(X, labels):
    s = silhouette_samples_ref(X, labels)
    return float(s.astype(np.float64).sum() / s.size)
