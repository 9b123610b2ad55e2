"""The exact shortcuts on data that defeats the fp16-split filter.

The accelerated sweeps are exact by construction: pruning skips only centroid groups that provably cannot win, the
fp16-split filter (csrc/filter.hip) settles a row only when its runner-up is provably out of reach, and every row it
cannot settle is redone in fp32.  What each layer settles depends on the data, so the suite's clean clips (about 1 % of
rows listed for the redo) leave most of the redo machinery idle.  These tests feed it data that it cannot settle:

1. noise-dominated clips (synth_clips(noisy=True), bench.py's `hard_workload`) through the whole pipeline, against the
   oracle at small sizes and against the plain dense fp32 sweeps at the full Lloyd shape;
2. data scaled down far enough that the filter's absolute error term lists every row, which walks a filtered exact call
   through each of its four ways to finish (csrc/exact_search.cpp; the route is exact_plan::plan in csrc/exact_plan.h):
     path 1  asynchronous form, short list: the redo kernels read the list length on the device
     path 2  asynchronous form, a list longer than n/16: the same kernels stride over it; the call's statistics then
             switch the context to the synchronous form (force_sync of the filter's totals)
     path 3  synchronous form, short list: exact_rows_kernel on the contiguous list; clears force_sync
     path 4  synchronous form, long list: the listed rows gathered (padded to at least 64), a fresh pre-pass and the
             fp32 MFMA pruned sweep over them
   and the fp16-range edge of the filter's input check (|v|^2 < 2^30);
3. the overlapped log-mel of DevicePipeline.run with waves that have to be converted first.

Every result is compared bit for bit with the oracle's fp32 contract, or with the same run on plain dense sweeps where
the oracle cannot finish in a test (the suite pins those to the oracle elsewhere)."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TINY = 1e-3          # rows and centroids x 1e-3: gaps below the filter's absolute error term, (nearly) every row listed


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device_frames(be, wave, n_mels, chunk=400):
    """The unit-norm frame-major rows the pipeline computes, on the host (the oracle is fed the device's frames: the
    log-mel is held to its tolerance elsewhere, everything after it is bit-exact by contract)."""
    T = be.num_frames(wave.shape[1], 128)
    out = np.empty((wave.shape[0] * T, n_mels), np.float32)
    for c0 in range(0, wave.shape[0], chunk):
        c1 = min(wave.shape[0], c0 + chunk)
        out[c0 * T:c1 * T] = be.logmel(wave[c0:c1], n_mels=n_mels, frame_major=True, l2norm=True).cpu().numpy()
    return out


def _oracle_pipeline(oracle, frames, T, n_train, k, niter, batch_clips):
    """ClusterCreator.run's batch loop and SpecTokenizer's search on host frames -> (centroids, tokens of all frames)."""
    cent = None
    for c0 in range(0, n_train, batch_clips):
        c1 = min(n_train, c0 + batch_clips)
        cent = oracle.kmeans_train(frames[c0 * T:c1 * T], k, niter=niter, init_centroids=cent).centroids
    cent = oracle.l2norm_rows(cent)
    return cent, oracle.assign(frames, cent)[0]


def _settle(be, xt, ct, order, cperm, dmin):
    """A filtered exact call on data the filter settles, then the statistics: leaves force_sync cleared (a short
    list clears it in the synchronous form and never sets it in the asynchronous one), whatever came before."""
    be.assign_pruned(xt, ct, order, cperm, dmin, filter=True)
    rows, listed = be.filter_stats()
    assert listed * 16 <= rows


# ---------------------------------------------------------------------------------------------------------------------
# 1. noise-dominated clips through the whole pipeline

@pytest.mark.parametrize("n_mels", [64, 128])
def test_noisy_clips_pipeline_against_the_oracle(be, oracle, n_mels):
    """150 noisy ten-second train clips in k-means batches of 60 (three trainings, two warm-started, the later batches'
    log-mel beside the training) and 12 validation clips, vocab 1024: every centroid and every token equal to the
    oracle's on the device's frames."""
    from audio_tokens_amd.pipeline import DevicePipeline
    from audio_tokens_amd.synth import synth_clips
    n_tr, n_va, k, niter = 150, 12, 1024, 8
    wave = synth_clips(n_tr + n_va, L=220500, seed=31, device=be.device, noisy=True)
    pipe = DevicePipeline(n_mels=n_mels, vocab_size=k, niter=niter, clustering_batch_size=60, backend=be)
    assert pipe.overlaps_logmel(n_tr)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        be.filter_stats()
        res = pipe.run(wave[:n_tr], wave[n_tr:])
        rows, listed = be.filter_stats()
        T = res.frames_per_clip
        frames = _device_frames(be, wave, n_mels)
        cent, ids = _oracle_pipeline(oracle, frames, T, n_tr, k, niter, 60)
    print(f"\nMEASURE noisy pipeline n_mels={n_mels}: listed {listed} of {rows} filtered rows ({listed / rows:.4f})")
    assert [len(s) for s in res.kmeans_stats] == [niter] * 3
    assert np.array_equal(bits(res.centroids.cpu().numpy()), bits(cent))
    assert np.array_equal(res.tokens_train.cpu().numpy(), ids[:n_tr * T])
    assert np.array_equal(res.tokens_val.cpu().numpy(), ids[n_tr * T:])


def test_noisy_clips_small_vocabulary_against_the_oracle(be, oracle):
    """configs[1]'s shape on noisy clips: vocab 500 (k-means unpruned, Lloyd on a 128 000-row subsample; tokenise
    through assign_unguided, the fp16-split filter with every group visited) -- every token equal to the oracle's."""
    from audio_tokens_amd.pipeline import DevicePipeline
    from audio_tokens_amd.synth import synth_clips
    n_tr, n_va, k, niter = 260, 40, 500, 10
    wave = synth_clips(n_tr + n_va, L=220500, seed=37, device=be.device, noisy=True)
    pipe = DevicePipeline(n_mels=64, vocab_size=k, niter=niter, clustering_batch_size=10000, backend=be)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        be.filter_stats()
        res = pipe.run(wave[:n_tr], wave[n_tr:])
        rows, listed = be.filter_stats()
        T = res.frames_per_clip
        frames = _device_frames(be, wave, 64)
        cent, ids = _oracle_pipeline(oracle, frames, T, n_tr, k, niter, 10000)
    print(f"\nMEASURE noisy vocab 500: listed {listed} of {rows} filtered rows")
    assert rows >= n_tr * T                             # (the tokeniser went through the filter sweep)
    assert np.array_equal(bits(res.centroids.cpu().numpy()), bits(cent))
    assert np.array_equal(res.tokens_train.cpu().numpy(), ids[:n_tr * T])
    assert np.array_equal(res.tokens_val.cpu().numpy(), ids[n_tr * T:])


# rows listed for the redo on these noisy clips, measured on an MI355X: 0.0361 (n_mels 64) and 0.0735 (n_mels 128) of
# the filtered rows of the accelerated run; the floors are half of that
NOISY_LISTED_FLOOR = {64: 0.018, 128: 0.036}


@pytest.mark.parametrize("n_mels", [64, 128])
def test_noisy_clips_full_lloyd_shape_accelerated_equals_dense(be, n_mels):
    """The full Lloyd shape on noisy clips: 1 220 ten-second train clips in the first k-means batch (2 102 060 frames,
    subsampled to 2 097 152 by the device permutation), a warm-started second batch of 300, 100 validation clips,
    vocab 8192, 20 iterations.  Pruning + filter + overlapped log-mel against plain dense sweeps: centroids, every
    token, every iteration's objective and repair count equal.  The data must keep reaching the redo: the listed
    fraction of the accelerated run is held above NOISY_LISTED_FLOOR (measured 0.036 at n_mels 64 and 0.074 at 128;
    clean clips list about 0.009)."""
    from audio_tokens_amd.pipeline import DevicePipeline
    from audio_tokens_amd.synth import synth_clips
    n_tr, n_va, k, niter, batch = 1520, 100, 8192, 20, 1220
    wave = synth_clips(n_tr + n_va, L=220500, seed=41, device=be.device, noisy=True)
    runs = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for prune in (True, False):
            pipe = DevicePipeline(n_mels=n_mels, vocab_size=k, niter=niter, clustering_batch_size=batch, backend=be,
                                  prune=prune)
            assert pipe.overlaps_logmel(n_tr) == prune
            be.filter_stats()
            runs[prune] = pipe.run(wave[:n_tr], wave[n_tr:])
            if prune:
                rows, listed = be.filter_stats()
    a, b = runs[True], runs[False]
    print(f"\nMEASURE noisy full shape n_mels={n_mels}: listed {listed} of {rows} filtered rows ({listed / rows:.4f})")
    assert 1220 * a.frames_per_clip > 256 * k
    assert torch.equal(a.centroids.view(torch.int32), b.centroids.view(torch.int32))
    assert torch.equal(a.tokens_train, b.tokens_train) and torch.equal(a.tokens_val, b.tokens_val)
    assert [len(s) for s in a.kmeans_stats] == [niter, niter]
    for sa, sb in zip(a.kmeans_stats, b.kmeans_stats):
        assert [s["obj"] for s in sa] == [s["obj"] for s in sb]
        assert [s["nsplit"] for s in sa] == [s["nsplit"] for s in sb]
    assert rows > 0 and listed / rows > NOISY_LISTED_FLOOR[n_mels]


# ---------------------------------------------------------------------------------------------------------------------
# 2. every finishing path of a filtered exact call

def _clustered(rng, n, k, d, oracle):
    centers = oracle.l2norm_rows(rng.standard_normal((k, d)).astype(np.float32))
    x = oracle.l2norm_rows((centers[rng.integers(0, k, n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32))
    c = oracle.l2norm_rows((centers + 0.01 * rng.standard_normal((k, d))).astype(np.float32))
    c[k // 2: k // 2 + 20] = c[0:20]                  # duplicated centroids: the lower index wins
    x[:20] = c[k // 2: k // 2 + 20]
    return x, c


def _pruned_inputs(be, oracle, x, c, rng):
    """Device tensors, oracle answer, and the pruning inputs of a guided exact call (guesses right for 4 rows in 5)."""
    ids_o, dis_o = oracle.assign(x, c)
    xt, ct = be._f32(x), be._f32(c)
    k = c.shape[0]
    hint = np.where(rng.random(x.shape[0]) < 0.2, rng.integers(0, k, x.shape[0]), ids_o)
    order = be.visit_order(torch.from_numpy(hint).to(be.device).contiguous(), None, k)
    cperm = be.from_host(be.group_rows_kd(c))
    dmin = be.group_min_dist(ct, cperm)
    return (xt, ct, order, cperm, dmin), (ids_o, dis_o)


# call -> (data, the list is longer than n/16, the path it takes)
PATH_SEQUENCE = [("tiny", True, 2), ("tiny", True, 4), ("unit", False, 3), ("unit", False, 1), ("tiny", True, 2)]


@pytest.mark.parametrize("d,k", [(64, 1024), (64, 8192), (128, 1024), (128, 8192)])
def test_filtered_calls_walk_every_finishing_path(be, oracle, switches, d, k):
    """Unit and tiny-scale batches on the same clustered data, called in the order tiny, tiny, unit, unit, tiny on one
    context with the statistics read after each call (which resolves the ring, so the form of the next call is known):
    paths 2, 4, 3, 1, 2.  Each call's list length is asserted on the side of n/16 its path needs, and every id and
    distance must be the oracle's; then the whole sequence again with ids only (want_dist=False, as tokenise calls)."""
    n = 70000
    rng = np.random.default_rng(d * 7 + k)
    x, c = _clustered(rng, n, k, d, oracle)
    data = {"unit": _pruned_inputs(be, oracle, x, c, rng),
            "tiny": _pruned_inputs(be, oracle, x * np.float32(TINY), c * np.float32(TINY), rng)}
    for want_dist in (True, False):
        _settle(be, *data["unit"][0])
        for i, (label, long_list, path) in enumerate(PATH_SEQUENCE):
            args, (ids_o, dis_o) = data[label]
            ids, dis = be.assign_pruned(*args, want_dist=want_dist, filter=True)
            rows, listed = be.filter_stats()
            what = f"call {i} ({label}, path {path}, want_dist={want_dist})"
            assert rows == n, what
            assert (listed * 16 > n) == long_list, f"{what}: listed {listed} of {n}"
            assert np.array_equal(ids.cpu().numpy(), ids_o), f"{what}: {(ids.cpu().numpy() != ids_o).sum()} ids differ"
            if want_dist:
                assert np.array_equal(bits(dis.cpu().numpy()), bits(dis_o)), what
            else:
                assert dis is None
    _settle(be, *data["unit"][0])


@pytest.mark.parametrize("d", [64, 128])
def test_long_list_path_at_small_n(be, oracle, switches, d):
    """Tiny-scale data at n = 20 ... 1000: the long-list redo gathers the listed rows and pads them to at least 64 by
    repeating the last one (at_filter_gather_ambiguous), so below 64 rows the pre-pass and the fp32 sweep run over rows
    that are not there.  Under filter_sync=1 every call takes the synchronous form (path 4); by default the first call
    is asynchronous (path 2) and the next synchronous (path 4).  Ids and distances must be the oracle's."""
    k = 1024
    rng = np.random.default_rng(d + 99)
    c = oracle.l2norm_rows(rng.standard_normal((k, d)).astype(np.float32))
    xu = oracle.l2norm_rows(rng.standard_normal((1000, d)).astype(np.float32))
    unit_args, _ = _pruned_inputs(be, oracle, *_clustered(rng, 2048, k, d, oracle), rng)
    for n in (20, 33, 63, 64, 65, 100, 1000):
        x = xu[:n] * np.float32(TINY)
        args, (ids_o, dis_o) = _pruned_inputs(be, oracle, x, c * np.float32(TINY), rng)
        for form in ("sync", "default"):
            switches(filter_sync=1 if form == "sync" else 0)
            _settle(be, *unit_args)
            # (default form: the first call is asynchronous, path 2; it switches the context to the synchronous form)
            for want_dist in (True, False, True):
                ids, dis = be.assign_pruned(*args, want_dist=want_dist, filter=True)
                rows, listed = be.filter_stats()
                what = f"n={n} {form} want_dist={want_dist}"
                assert rows == n and listed * 16 > n, f"{what}: listed {listed}"
                assert np.array_equal(ids.cpu().numpy(), ids_o), what
                if want_dist:
                    assert np.array_equal(bits(dis.cpu().numpy()), bits(dis_o)), what
    switches(filter_sync=0)
    _settle(be, *unit_args)


def _big(v0, v1=0.0, d=64):
    r = np.zeros(d, np.float32)
    r[0], r[1] = np.float32(v0), np.float32(v1)
    return r


@pytest.mark.parametrize("d", [64, 128])
def test_fp16_range_boundary(be, oracle, d):
    """The filter takes a row or a centroid only if its squared norm is below 2^30 (every component then fits fp16);
    a row at or past the edge is listed, a centroid at or past it lists every row.  On well separated data at 2^14 scale
    (which the filter settles completely) one row or centroid is set to: |v|^2 one ulp below 2^30 (2^30 - 64), exactly
    2^30, one component one ulp below 2^15, one component one ulp above.  Listed counts as intended, results the
    oracle's."""
    k, n = 1024, 4096
    rng = np.random.default_rng(d + 5)
    s = np.float32(2.0 ** 14)
    c = oracle.l2norm_rows(rng.standard_normal((k, d)).astype(np.float32)) * s
    c[0] = _big(2.0 ** 14, d=d)
    x = (c[rng.integers(0, k, n)] + s * np.float32(0.02) * rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
    below = np.float32(2.0 ** 15) - np.float32(2.0 ** -9)          # the float below 2^15
    above = np.float32(2.0 ** 15) + np.float32(2.0 ** -8)          # the float above it
    assert np.float32(below * below) + np.float32(64) == np.nextafter(np.float32(2.0 ** 30), np.float32(0))
    cases = [("row", "norm^2 2^30 - 64", _big(below, 8.0, d), False), ("row", "norm^2 2^30", _big(2.0 ** 15, d=d), True),
             ("row", "component below 2^15", _big(below, d=d), False), ("row", "component above 2^15", _big(above, d=d), True),
             ("centroid", "norm^2 2^30 - 64", _big(below, 8.0, d), False),
             ("centroid", "norm^2 2^30", _big(2.0 ** 15, d=d), True),
             ("centroid", "component below 2^15", _big(below, d=d), False),
             ("centroid", "component above 2^15", _big(above, d=d), True)]
    for where, label, v, out_of_range in [("none", "base", None, False)] + cases:
        xx, cc = x.copy(), c.copy()
        if where == "row":
            xx[7] = v
        elif where == "centroid":
            cc[1] = v
        args, (ids_o, dis_o) = _pruned_inputs(be, oracle, xx, cc, rng)
        ids, dis = be.assign_pruned(*args, filter=True)
        rows, listed = be.filter_stats()
        assert np.array_equal(ids.cpu().numpy(), ids_o), (where, label)
        assert np.array_equal(bits(dis.cpu().numpy()), bits(dis_o)), (where, label)
        want = (n if where == "centroid" else 1) if out_of_range else 0
        assert rows == n and listed == want, f"{where} {label}: listed {listed}, expected {want}"
    _settle(be, *_pruned_inputs(be, oracle, x, c, rng)[0])


@pytest.mark.parametrize("d", [64, 128])
def test_training_across_filter_regimes(be, oracle, d):
    """Kmeans.train (k = 2048, 70 000 rows cold, then 40 000 warm-started, 6 iterations) on unit data, on tiny-scale
    data (every row listed: the asynchronous calls switch the context to the synchronous form while iterations are
    queued) and at 3e-3 scale (about a fifth listed: the form flips back and forth inside a training), then on unit
    data again.  Measured listed fractions on an MI355X: unit 0.0022 / 0.0063 (d = 64 / 128), tiny 1.0, 3e-3 0.199 /
    0.210.  Centroids and repair counts equal to the oracle's and, with the objectives, to the same
    trainings on plain dense sweeps; each scale's listed fraction asserted, so the test proves which regime it ran in.
    The second unit training must list exactly what the first did (the listing does not depend on the form)."""
    from audio_tokens_amd.ops import Kmeans
    k, n1, n2, niter = 2048, 70000, 40000, 6
    rng = np.random.default_rng(d)
    cen = rng.standard_normal((k, d))
    x = oracle.l2norm_rows((cen[rng.integers(0, k, n1 + n2)] + 0.5 * rng.standard_normal((n1 + n2, d))).astype(np.float32))
    regimes = [("unit", 1.0, 0.0, 1 / 32), ("tiny", TINY, 0.5, 1.0), ("3e-3", 3e-3, 1 / 32, 1 / 4), ("unit again", 1.0, 0.0, 1 / 32)]
    seen, ref = {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for label, scale, lo, hi in regimes:
            xs = (x * np.float32(scale)).astype(np.float32)
            if scale not in ref:
                r1 = oracle.kmeans_train(xs[:n1], k, niter=niter)
                r2 = oracle.kmeans_train(xs[n1:], k, niter=niter, init_centroids=r1.centroids)
                ref[scale] = (r1, r2)
            r1, r2 = ref[scale]
            got = {}
            for prune in (True, False):
                km = Kmeans(d, k, niter=niter, backend=be)
                km.prune = prune
                be.filter_stats()
                km.train(xs[:n1])
                cold = (km.centroids.copy(), list(km.obj), [s["nsplit"] for s in km.iteration_stats])
                km.train(xs[n1:], init_centroids=km.centroids)
                got[prune] = cold + (km.centroids.copy(), list(km.obj), [s["nsplit"] for s in km.iteration_stats])
                if prune:
                    rows, listed = be.filter_stats()
            frac = listed / rows
            seen[label] = (rows, listed)
            print(f"\nMEASURE training d={d} {label}: listed {listed} of {rows} filtered rows ({frac:.4f})")
            a, b = got[True], got[False]
            assert np.array_equal(bits(a[0]), bits(r1.centroids)), f"{label} cold"
            assert a[2] == list(r1.nsplit), label
            assert np.allclose(a[1], r1.obj, rtol=2e-5, atol=0), label
            assert np.array_equal(bits(a[3]), bits(r2.centroids)), f"{label} warm"
            assert a[5] == list(r2.nsplit), label
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[3]), bits(b[3])), label
            assert a[1] == b[1] and a[2] == b[2] and a[4] == b[4] and a[5] == b[5], label
            assert lo <= frac <= hi, f"{label}: listed fraction {frac:.4f} outside [{lo:.4f}, {hi:.4f}]"
    assert seen["unit again"] == seen["unit"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. the overlapped log-mel with waves that need converting

def _hold_back_the_main_stream(monkeypatch):
    """Queues a delay on the main stream in front of the first batch's log-mel, so that the side stream's launches and the
    main stream's next work are all queued before either starts: what happens to a freed block is then decided by the
    stream order, not by how fast the host gets there."""
    from audio_tokens_amd.pipeline import DevicePipeline
    frames_beside = DevicePipeline._frames_beside

    def delayed(self, *args, **kw):
        torch.cuda._sleep(50_000_000)
        return frames_beside(self, *args, **kw)
    monkeypatch.setattr(DevicePipeline, "_frames_beside", delayed)


def _converted_kinds(wave):
    big = torch.zeros((wave.shape[0], wave.shape[1] + 16), dtype=torch.float32, device=wave.device)
    big[:, 7:7 + wave.shape[1]] = wave
    return {"host fp32": wave.cpu(), "device fp64": wave.double(), "strided device fp32": big[:, 7:7 + wave.shape[1]]}


def test_logmel_beside_the_training_with_converted_waves(be, monkeypatch):
    """DevicePipeline.run converts host, float64 and strided waves into temporaries on the main stream; in the overlapped
    form the side stream reads them after the frames helper returned.  The first train() call here at once allocates
    tensors of the converted waves' sizes on the main stream and fills them with NaN: were the temporaries already
    freed, those would be their blocks, and the side stream (held back behind the first batch by a delay on the main
    stream) would make frames of NaN.  Same centroids and tokens as the contiguous device fp32 wave, overlap on and off.
    (Against the form that let the temporaries go, this failed with faiss' isfinite error.)"""
    from audio_tokens_amd import ops
    from audio_tokens_amd.pipeline import DevicePipeline
    from audio_tokens_amd.synth import synth_clips
    wave = synth_clips(27, L=22050 * 2, seed=11, device="cuda")
    pipe = DevicePipeline(n_mels=64, vocab_size=1024, niter=4, clustering_batch_size=6, backend=be)
    pipe.beside_clips = 2
    assert pipe.overlaps_logmel(24)
    train, held = ops.Kmeans.train, []

    def train_after_claiming_freed_blocks(self, x, *args, **kw):
        if not held:
            for shape in ((24, wave.shape[1]), (3, wave.shape[1])):
                held.append(torch.full(shape, float("nan"), dtype=torch.float32, device=be.device))
        return train(self, x, *args, **kw)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = pipe.run(wave[:24], wave[24:])
        pipe.overlap_logmel = False
        seq = pipe.run(wave[:24], wave[24:])
        pipe.overlap_logmel = True
        assert torch.equal(ref.centroids.view(torch.int32), seq.centroids.view(torch.int32))
        assert torch.equal(ref.tokens_train, seq.tokens_train) and torch.equal(ref.tokens_val, seq.tokens_val)
        monkeypatch.setattr(ops.Kmeans, "train", train_after_claiming_freed_blocks)
        _hold_back_the_main_stream(monkeypatch)
        for name, wv in _converted_kinds(wave).items():
            for overlap in (True, False):
                pipe.overlap_logmel = overlap
                held.clear()
                got = pipe.run(wv[:24], wv[24:])
                assert len(held) == 2
                what = f"{name}, overlap {overlap}"
                assert torch.equal(got.centroids.view(torch.int32), ref.centroids.view(torch.int32)), what
                assert torch.equal(got.tokens_train, ref.tokens_train), what
                assert torch.equal(got.tokens_val, ref.tokens_val), what


def test_logmel_beside_a_failing_training_leaves_no_writer_behind(be, monkeypatch):
    """A train() that raises while the side stream still has log-mel launches queued: run() must not let the frames go
    back to the allocator before the main stream has waited for them.  A tensor of the training frames' size allocated
    right after the exception (no synchronisation in between) and filled with a sentinel must keep it.  (Against the form
    without that wait, 397 440 of its values were overwritten by the side stream's frames.)"""
    from audio_tokens_amd import ops
    from audio_tokens_amd.pipeline import DevicePipeline
    from audio_tokens_amd.synth import synth_clips
    wave = synth_clips(27, L=22050 * 2, seed=11, device="cuda")
    pipe = DevicePipeline(n_mels=64, vocab_size=1024, niter=4, clustering_batch_size=6, backend=be)
    pipe.beside_clips = 2
    assert pipe.overlaps_logmel(24)
    T = be.num_frames(wave.shape[1], 128)
    pipe.run(wave[:24], wave[24:])                     # (the context's side stream and caches exist)
    torch.cuda.synchronize()

    def failing_train(self, x, *args, **kw):
        raise RuntimeError("training failed on purpose")

    monkeypatch.setattr(ops.Kmeans, "train", failing_train)
    _hold_back_the_main_stream(monkeypatch)
    failed = False
    try:
        pipe.run(wave[:24], wave[24:])
    except RuntimeError as e:
        failed = "on purpose" in str(e)
    assert failed
    sentinel = torch.full((24 * T, 64), 12345.0, dtype=torch.float32, device=be.device)
    torch.cuda.synchronize()
    assert bool((sentinel == 12345.0).all()), f"{int((sentinel != 12345.0).sum())} values overwritten after the failure"
