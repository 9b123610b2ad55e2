"""at_frontend_plan_host through ctypes (no GPU): the layout of a batch of clips of unequal length, channel count and
sample rate for the ragged front end, on hand-computed cases."""
import numpy as np
import pytest

from audio_tokens_amd import _lib


@pytest.fixture(scope="module")
def host():
    from audio_tokens_amd.backend import HostHelpers
    return HostHelpers()


def test_hand_computed_batch(host):
    # n_fft = 512, hop = 128, all at 22050: lengths 1000, 256 (too short), 257 (shortest valid), 1281
    plan, order, groups, tot = host.frontend_plan([1, 2, 1, 1], [1000, 256, 257, 1281], [22050] * 4, 22050, 512, 128)
    assert plan["out_length"].tolist() == [1000, 256, 257, 1281]
    assert plan["too_short"].tolist() == [0, 1, 0, 0]
    assert plan["n_frames"].tolist() == [1 + 1000 // 128, 0, 1 + 257 // 128, 1 + 1281 // 128] == [8, 0, 3, 11]
    assert plan["first_frame"].tolist() == [0, 8, 8, 11]               # exclusive prefix sums
    assert plan["mono_offset"].tolist() == [0, 1000, 1256, 1516]        # 257 -> 260 floats
    assert (plan["mono_offset"] % 4 == 0).all()
    assert plan["first_block16"].tolist() == [0, 1, 1, 2] and plan["first_block32"].tolist() == [0, 1, 1, 2]
    assert plan["in_offset"].tolist() == [0, 1000, 1512, 1769]          # blocks back to back: the stereo clip takes 512
    assert plan["channels"].tolist() == [1, 2, 1, 1]
    assert tot == {"mono_floats": 1516 + 1284, "n_frames": 22, "n_blocks16": 3, "n_blocks32": 3, "n_short": 1, "n_groups": 1}
    assert len(groups) == 1 and groups[0]["mode"] == _lib.AT_FRONTEND_COPY and groups[0]["K"] == 0
    assert groups[0]["first"] == 0 and groups[0]["count"] == 4 and order.tolist() == [0, 1, 2, 3]
    # one workgroup of the copy kernel per clip (4096 samples each)
    assert plan["rs_first_block"].tolist() == [0, 1, 2, 3] and groups[0]["n_blocks"] == 4


def test_row_offsets_are_rounded_up_to_four_floats(host):
    lengths = [33, 34, 35, 36, 37, 1]
    plan, _, _, tot = host.frontend_plan([1] * 6, lengths, [16000] * 6, 16000, 64, 64)
    assert plan["mono_offset"].tolist() == [0, 36, 72, 108, 144, 184]
    assert tot["mono_floats"] == 188


@pytest.mark.parametrize("n_fft", [64, 512, 400])
def test_too_short_is_marked_at_half_the_transform(host, n_fft):
    half = n_fft // 2
    plan, _, _, tot = host.frontend_plan([1, 1], [half, half + 1], [22050, 22050], 22050, n_fft, 16)
    assert plan["too_short"].tolist() == [1, 0]
    assert plan["n_frames"].tolist() == [0, host.num_frames(half + 1, 16)]
    assert plan["first_frame"].tolist() == [0, 0] and tot["n_short"] == 1
    # after resampling: 2 * half + 1 input samples at twice the rate give ceil((2 * half + 1) / 2) = half + 1
    plan, _, _, _ = host.frontend_plan([1, 1], [2 * half, 2 * half + 1], [44100, 44100], 22050, n_fft, 16)
    assert plan["out_length"].tolist() == [half, half + 1] and plan["too_short"].tolist() == [1, 0]


def test_clips_are_grouped_by_reduced_rate_pair(host):
    # 44100 -> 22050 and 48000 -> 24000 reduce to (2, 1): one group, although the rates differ
    for common, rates in ((22050, [44100, 22050, 44100, 16000, 22050, 48000]),):
        plan, order, groups, tot = host.frontend_plan([1] * 6, [3000] * 6, rates, common, 512, 128)
        assert plan["group"].tolist() == [0, 1, 0, 2, 1, 3]              # in order of first appearance
        assert [(g["orig"], g["nw"]) for g in groups] == [(2, 1), (1, 1), (320, 441), (320, 147)]
        assert order.tolist() == [0, 2, 1, 4, 3, 5]
        assert [(int(g["first"]), int(g["count"])) for g in groups] == [(0, 2), (2, 2), (4, 1), (5, 1)]
        for g, (of, nf) in zip(groups, [(44100, 22050), (22050, 22050), (16000, 22050), (48000, 22050)]):
            _, o, n, w = host.resample_taps(of, nf) if of != nf else (None, 1, 1, 0)
            assert (g["orig"], g["nw"], g["width"]) == (o, n, w)
            assert g["K"] == (2 * w + o if of != nf else 0)
        assert plan["out_length"].tolist() == [host.resample_length(3000, r, common) for r in rates]
    a = host.frontend_plan([1], [3000], [44100], 22050, 512, 128)[2][0]
    b = host.frontend_plan([1], [3000], [48000], 24000, 512, 128)[2][0]
    for name in ("orig", "nw", "width", "K", "mode", "TI", "out_per_block", "n_blocks"):
        assert a[name] == b[name], name
    assert (a["orig"], a["nw"]) == (2, 1) and a["mode"] == _lib.AT_FRONTEND_TILED
    # the tile is what at_resample_f32 uses: as many input steps as fit 8192 floats of LDS, a multiple of 4
    fit = (8192 - a["K"]) // 2 + 1
    assert a["TI"] == fit - fit % 4 and a["out_per_block"] == a["TI"]
    assert a["n_blocks"] == -(-1500 // int(a["TI"]))


def test_resampler_blocks_are_counted_within_the_group(host):
    rates = [44100, 22050, 44100, 44100]
    lengths = [20000, 9000, 2, 30000]
    plan, _, groups, _ = host.frontend_plan([1, 2, 1, 2], lengths, rates, 22050, 512, 128)
    ti = int(groups[0]["TI"])
    blocks = [-(-10000 // ti), -(-1 // ti), -(-15000 // ti)]
    assert plan["rs_first_block"].tolist() == [0, 0, blocks[0], blocks[0] + blocks[1]]
    assert groups[0]["n_blocks"] == sum(blocks)
    assert groups[1]["n_blocks"] == -(-9000 // 4096) and groups[1]["out_per_block"] == 4096


def test_totals_are_int64(host):
    # 3 clips of 2^31 - 2 samples at hop 1: 2^31 - 1 frames each, their sum and the buffer past 2^32 (plan only)
    L = 2 ** 31 - 2
    plan, _, _, tot = host.frontend_plan([1, 1, 1], [L] * 3, [22050] * 3, 22050, 64, 1)
    T = L + 1
    assert plan["n_frames"].tolist() == [T] * 3
    assert plan["first_frame"].tolist() == [0, T, 2 * T] and tot["n_frames"] == 3 * T > 2 ** 32
    assert plan["mono_offset"].tolist() == [0, L + 2, 2 * (L + 2)] and tot["mono_floats"] == 3 * (L + 2)
    assert tot["n_blocks16"] == 3 * (-(-T // 16)) and tot["n_blocks32"] == 3 * (-(-T // 32))
    # one frame more per clip does not fit the kernels' int frame index
    with pytest.raises(_lib.NativeError, match="too many frames"):
        host.frontend_plan([1], [L + 1], [22050], 22050, 64, 1)


def test_zero_clips(host):
    plan, order, groups, tot = host.frontend_plan([], [], [], 22050, 512, 128)
    assert len(plan) == 0 and len(order) == 0 and len(groups) == 0
    assert tot == {"mono_floats": 0, "n_frames": 0, "n_blocks16": 0, "n_blocks32": 0, "n_short": 0, "n_groups": 0}


def test_seventy_thousand_clips(host):
    n = 70_000
    rng = np.random.default_rng(5)
    lengths = rng.choice([33, 100, 200], n)
    rates = rng.choice([22050, 44100], n)
    ch = rng.choice([1, 2], n)
    plan, order, groups, tot = host.frontend_plan(ch, lengths, rates, 22050, 64, 64)
    out_len = np.where(rates == 44100, (lengths + 1) // 2, lengths)
    T = np.where(out_len > 32, 1 + out_len // 64, 0)
    assert np.array_equal(plan["out_length"], out_len) and np.array_equal(plan["n_frames"], T)
    assert np.array_equal(plan["first_frame"], np.cumsum(T) - T) and tot["n_frames"] == T.sum()
    pad = (out_len + 3) // 4 * 4
    assert np.array_equal(plan["mono_offset"], np.cumsum(pad) - pad) and tot["mono_floats"] == pad.sum()
    assert tot["n_short"] == (out_len <= 32).sum() > 0 and len(groups) == 2
    assert sorted(order.tolist()) == list(range(n))
    for g, grp in enumerate(groups):
        mine = order[grp["first"]: grp["first"] + grp["count"]]
        assert (plan["group"][mine] == g).all() and (np.diff(mine) > 0).all()
        assert np.array_equal(plan["rs_first_block"][mine], np.arange(len(mine)))   # one block each at these lengths


def test_bad_arguments_are_refused(host):
    with pytest.raises(_lib.NativeError, match="channels"):
        host.frontend_plan([3], [1000], [22050], 22050, 512, 128)
    with pytest.raises(_lib.NativeError, match="rate"):
        host.frontend_plan([1], [1000], [0], 22050, 512, 128)
    with pytest.raises(_lib.NativeError, match="row_stride"):
        host.frontend_plan([2], [1000], [22050], 22050, 512, 128, offsets=[0], row_strides=[999])
