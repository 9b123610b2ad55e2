"""CPU checks of the silhouette yardstick (tests/silhouette_ref.py) against sklearn, and of the library's export."""
import ctypes

import numpy as np
import pytest

from silhouette_ref import silhouette_samples_ref, silhouette_score_ref


def _cases():
    rng = np.random.default_rng(7)
    # blobs
    cen = rng.normal(size=(5, 16)).astype(np.float32) * 3
    lab = rng.integers(0, 5, 400)
    yield "blobs", (cen[lab] + rng.normal(size=(400, 16))).astype(np.float32), lab
    # unit rows with singletons, duplicates across clusters, a cluster of identical rows, negative and sparse labels
    x = rng.normal(size=(300, 64)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    lab = rng.choice(np.array([-7, -1, 3, 1000, 2**40]), 300)
    lab[:5] = [11, 12, 13, 14, 15]                 # five singletons
    x[40:60] = x[40]
    lab[40:60] = 99                                # identical rows, one cluster
    x[100] = x[200]                                # exact duplicates in different clusters
    lab[100], lab[200] = -7, 3
    yield "mixed", x, lab
    # about 1.2 rows per cluster
    n = 240
    yield "sparse", rng.normal(size=(n, 3)).astype(np.float32), rng.integers(0, 200, n)
    # one dimension
    yield "d1", rng.normal(size=(120, 1)).astype(np.float32), rng.integers(0, 4, 120)


@pytest.mark.parametrize("name", ["blobs", "mixed", "sparse", "d1"])
def test_reference_copy_equals_sklearn(name):
    sk = pytest.importorskip("sklearn.metrics")
    x, lab = {c[0]: c[1:] for c in _cases()}[name]
    mine = silhouette_samples_ref(x, lab)
    theirs = sk.silhouette_samples(x, lab)
    assert theirs.dtype == np.float32
    assert np.abs(mine.astype(np.float64) - theirs).max() <= 2e-6
    assert (mine.view(np.uint32) == theirs.view(np.uint32)).mean() > 0.9
    assert abs(silhouette_score_ref(x, lab) - sk.silhouette_score(x, lab)) <= 1e-6


def test_reference_copy_rejects_label_counts():
    x = np.zeros((4, 2), np.float32)
    with pytest.raises(ValueError, match="Number of labels is 1"):
        silhouette_samples_ref(x, [3, 3, 3, 3])
    with pytest.raises(ValueError, match="Number of labels is 4"):
        silhouette_samples_ref(x, [0, 1, 2, 3])


def test_library_exports_silhouette():
    from audio_tokens_amd import _lib
    if not _lib.LIB_PATH.exists():
        pytest.fail("the library is not built")
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(lib, "at_silhouette_f32")
    assert "at_silhouette_f32" in _lib.SIGNATURES
    assert _lib.load().at_silhouette_f32 is not None
