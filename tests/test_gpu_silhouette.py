"""at_silhouette_f32 / ops.silhouette_score on the MI355X against the fp64 yardsticks: tests/silhouette_ref.py (numpy),
sklearn where it imports, and a chunked torch fp64 copy of the same recipe on the GPU for the larger cases."""
import logging
import sys
import types

import numpy as np
import pytest
import torch

from silhouette_ref import silhouette_samples_ref, silhouette_score_ref

pytestmark = pytest.mark.gpu

S_TOL, SCORE_TOL = 2e-6, 1e-6


def _sklearn():
    try:
        import sklearn.metrics as sk
        return sk
    except Exception:
        return None


def _torch_fp64(x, labels, chunk=2048):
    """The recipe of silhouette_ref.py with torch on the device (fp64 cluster sums through index_add_)."""
    x64 = x.double()
    _, enc = torch.unique(labels, return_inverse=True)
    k = int(enc.max()) + 1
    freq = torch.bincount(enc, minlength=k).double()
    nrm = (x64 * x64).sum(1)
    n = x.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        d2 = ((-2.0 * (x64[i0:i1] @ x64.T)) + nrm[i0:i1, None]) + nrm[None, :]
        d2 = d2.float().clamp_min(0)
        r = torch.arange(i1 - i0, device=x.device)
        d2[r, r + i0] = 0
        dist = d2.double().sqrt().float().double()
        S = torch.zeros(i1 - i0, k, dtype=torch.float64, device=x.device).index_add_(1, enc, dist).float()
        own = enc[i0:i1]
        a = (S[r, own].double() / (freq[own] - 1)).float()
        S[r, own] = float("inf")
        b = (S.double() / freq).float().min(1).values
        s = ((b - a).double() / torch.maximum(a, b).double()).float()
        out[i0:i1] = torch.nan_to_num(s, nan=0.0)
    return out


def _labels(rng, n, k):
    lab = rng.integers(0, k, n)
    lab[: min(n, 2)] = [0, 1][: min(n, 2)]          # at least two labels
    return lab


def _blobs(rng, n, d, k):
    cen = rng.normal(size=(k, d)).astype(np.float32)
    lab = _labels(rng, n, k)
    return (cen[lab] + 0.7 * rng.normal(size=(n, d))).astype(np.float32), lab


def _check(be, x, lab, sk_too=True):
    s = be.to_host(be.silhouette_samples(x, lab))
    ref = silhouette_samples_ref(x, lab)
    assert np.abs(s.astype(np.float64) - ref).max() <= S_TOL
    total = be.empty((1,), torch.float64)
    be.silhouette_samples(x, lab, sum_out=total)
    assert abs(float(total.item()) / len(s) - silhouette_score_ref(x, lab)) <= SCORE_TOL
    sk = _sklearn()
    if sk is not None and sk_too:
        theirs = sk.silhouette_samples(x, lab)
        assert np.abs(s.astype(np.float64) - theirs).max() <= S_TOL
        return (s.view(np.uint32) == theirs.view(np.uint32)).mean()
    return None


@pytest.mark.parametrize("d", [1, 3, 64, 128, 640])
@pytest.mark.parametrize("n", [3, 17, 1000])
def test_matches_reference_and_sklearn(be, n, d):
    rng = np.random.default_rng(n * 1000 + d)
    x, lab = _blobs(rng, n, d, max(2, n // 8))
    _check(be, x, lab)


@pytest.mark.parametrize("d", [3, 64, 640])
def test_twenty_thousand_rows(be, d):
    rng = np.random.default_rng(d)
    x, lab = _blobs(rng, 20000, d, 40)
    _check(be, x, lab, sk_too=d == 64)


def test_about_one_row_per_cluster(be):
    rng = np.random.default_rng(5)
    x = rng.normal(size=(12000, 64)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    lab = rng.integers(0, 10000, 12000)          # ~1.2 rows per present label, many singletons
    share = _check(be, x, lab)
    assert share is None or share > 0.99


def test_identical_rows_duplicates_and_shuffled_labels(be):
    rng = np.random.default_rng(11)
    x, lab = _blobs(rng, 3000, 64, 7)
    lab = np.array([-5, 3, 17, 2**40, -2**40, 0, 9])[lab]   # negative, sparse, wide labels
    x[100:400] = x[100]
    lab[100:400] = 123                                     # a cluster of identical rows: a = 0 there
    x[1000:1010] = x[2000]                                 # exact duplicates in other clusters (distance 0, not i == j)
    perm = rng.permutation(3000)
    _check(be, x[perm], lab[perm])


def test_sixteen_clusters_65536_rows(be):
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(65536, 64, generator=g).to(be.device)
    lab = torch.randint(0, 16, (65536,), generator=g).to(be.device)
    x = x + 2.0 * torch.randn(16, 64, generator=g).to(be.device)[lab]
    s = be.silhouette_samples(x, lab)
    t = _torch_fp64(x, lab)
    assert (s.double() - t.double()).abs().max().item() <= S_TOL
    assert abs(s.double().mean().item() - t.double().mean().item()) <= SCORE_TOL


@pytest.fixture(scope="module")
def kmeans_frames(be):
    from audio_tokens_amd.ops import Kmeans
    from audio_tokens_amd.synth import synth_clips
    wave = synth_clips(380, L=22050, seed=99, device=be.device)
    frames = be.logmel(wave, n_mels=64, frame_major=True, l2norm=True)[:65536].contiguous()
    km = Kmeans(64, 8192, niter=2, backend=be)
    km.train(frames)
    ids, _ = be.assign(frames, be.l2norm_rows(km.centroids_device))
    return frames, ids


def test_kmeans_8192_labels_65536_rows(be, kmeans_frames):
    x, ids = kmeans_frames
    s = be.silhouette_samples(x, ids)
    t = _torch_fp64(x, ids)
    assert (s.double() - t.double()).abs().max().item() <= S_TOL
    assert abs(s.double().mean().item() - t.double().mean().item()) <= SCORE_TOL


def test_two_calls_give_the_same_bits(be, kmeans_frames):
    x, ids = kmeans_frames
    t1, t2 = be.empty((1,), torch.float64), be.empty((1,), torch.float64)
    s1 = be.silhouette_samples(x, ids, sum_out=t1).clone()
    s2 = be.silhouette_samples(x, ids, sum_out=t2)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert t1.item() == t2.item()


def test_rejects_label_counts_and_nonfinite_rows(be):
    x = np.random.default_rng(0).normal(size=(50, 8)).astype(np.float32)
    with pytest.raises(ValueError, match="Number of labels is 1. Valid values are 2 to n_samples - 1"):
        be.silhouette_samples(x, np.full(50, 7))
    with pytest.raises(ValueError, match="Number of labels is 50. Valid values are 2 to n_samples - 1"):
        be.silhouette_samples(x, np.arange(50))
    lab = np.arange(50) % 3
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[17, 5] = bad
        with pytest.raises(ValueError):
            be.silhouette_samples(y, lab)


def test_sampled_score_follows_sklearns_draw(be):
    from audio_tokens_amd.ops import silhouette_score
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(21)
    x, lab = _blobs(rng, 30000, 64, 50)
    np.random.seed(1234)
    want = sk.silhouette_score(x, lab, sample_size=10000)
    want_next = np.random.rand()
    np.random.seed(1234)
    got = silhouette_score(torch.from_numpy(x).to(be.device), lab, sample_size=10000)
    assert np.random.rand() == want_next
    assert abs(got - want) <= SCORE_TOL
    assert abs(silhouette_score(x, lab, sample_size=10000, random_state=5)
               - sk.silhouette_score(x, lab, sample_size=10000, random_state=5)) <= SCORE_TOL


def test_evaluate_clustering_needs_no_sklearn(be, monkeypatch):
    from audio_tokens_amd.processors.cluster_creator import ClusterCreator
    rng = np.random.default_rng(8)
    x, lab = _blobs(rng, 12000, 64, 30)
    np.random.seed(77)
    idx = np.random.permutation(12000)[:10000]
    want = silhouette_score_ref(x[idx], lab[idx])
    np.random.seed(77)
    monkeypatch.setitem(sys.modules, "sklearn", None)
    monkeypatch.setitem(sys.modules, "sklearn.metrics", None)
    got = ClusterCreator.evaluate_clustering(types.SimpleNamespace(logger=logging.getLogger("t")), x, lab)
    assert isinstance(got, float)
    assert abs(got - want) <= SCORE_TOL
