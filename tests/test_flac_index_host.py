"""HostHelpers.flac_index (at_flac_index_host) against the frame list the test encoder reports.  CPU only."""
import numpy as np
import pytest

import flac_ref as F


@pytest.fixture(scope="module")
def host():
    from audio_tokens_amd.backend import HostHelpers
    return HostHelpers()


def _smooth(C, L, seed, amp=3000):
    rng = np.random.default_rng(seed)
    return (np.sin(np.arange(L) * 0.02)[None, :] * amp + rng.integers(-8, 9, (C, L))).astype(np.int64)


def _check(host, data, frames, C, L, sr=44100, bps=16):
    facts, table = host.flac_index(data)
    assert (facts["channels"], facts["bits_per_sample"], facts["sample_rate"], facts["total_samples"]) == (C, bps, sr, L)
    assert len(table) == len(frames)
    for name in ("offset", "first_sample", "block_size"):
        assert table[name].tolist() == [f[name] for f in frames], name
    assert table["length"].tolist()[:-1] == [f["length"] for f in frames][:-1]
    assert (table["bits_per_sample"] == bps).all() and (table["channels"] == C).all()
    return facts, table


def test_fixed_blocksize_positions(host):
    frames = []
    x = _smooth(2, 5000, 0)
    data = F.encode(x, 44100, 16, block_size=1152, assignment="mid_side", frames_out=frames)
    facts, table = _check(host, data, frames, 2, 5000)
    assert facts["variable_blocksize"] == 0 and (table["channel_assignment"] == 10).all()
    assert int(table["length"][-1]) == frames[-1]["length"]
    assert table["block_size"].tolist() == [1152] * 4 + [392]


def test_variable_blocksize_positions(host):
    sizes = [16, 17, 192, 255, 256, 257, 576, 4096, 4608, 33]
    frames = []
    data = F.encode(_smooth(1, sum(sizes), 1), 22050, 16, block_size=sizes, frames_out=frames)
    facts, table = _check(host, data, frames, 1, sum(sizes), sr=22050)
    assert facts["variable_blocksize"] == 1 and (facts["min_block"], facts["max_block"]) == (16, 4608)


def test_frame_numbers_of_one_two_and_three_bytes(host):
    frames = []
    L = 2100 * 16                                # frame numbers pass 127 and 2047
    x = (np.arange(L) % 7 - 3)[None, :]
    data = F.encode(x, 8000, 8, block_size=16, subframe={"type": "verbatim"}, frames_out=frames)
    _, table = _check(host, data, frames, 1, L, sr=8000, bps=8)
    assert sorted(set(table["header_bytes"].tolist())) == [7, 8, 9]


def test_variable_stream_past_65535_samples(host):
    sizes = [65535, 4096, 17]
    frames = []
    x = np.zeros((1, sum(sizes)), np.int64)
    x[0, ::1000] = 5
    data = F.encode(x, 44100, 16, block_size=sizes, subframe={"type": "fixed", "order": 0, "param": 0}, frames_out=frames)
    _, table = _check(host, data, frames, 1, sum(sizes))
    assert table["first_sample"].tolist() == [0, 65535, 69631]


def test_id3_prefix_extra_metadata_and_trailing_junk(host):
    tag = b"\x00" * 300
    id3 = b"ID3\x04\x00\x00" + bytes([0, 0, 300 >> 7, 300 & 0x7F]) + tag
    vorbis = (4, (7).to_bytes(4, "little") + b"encoder" + (0).to_bytes(4, "little"))
    padding = (1, b"\xff\xf8" * 40)              # (a padding block is not searched for frames)
    frames = []
    x = _smooth(1, 1000, 2)
    data = F.encode(x, 44100, 16, block_size=256, frames_out=frames, prefix=id3, extra_metadata=(vorbis, padding),
                    suffix=b"TAG" + b"\x00" * 125)
    _, table = _check(host, data, frames, 1, 1000)
    assert int(table["offset"][0]) == len(id3) + 4 + 38 + 4 + len(vorbis[1]) + 4 + 80
    assert int(table["length"][-1]) == frames[-1]["length"] + 128       # a bound: up to the end of the data


@pytest.mark.parametrize("min_frame_known", [True, False])
def test_planted_sync_codes_are_not_frames(host, min_frame_known):
    # verbatim 16-bit samples are the payload's bytes: plant the sync pattern, and whole frame headers, in them
    rng = np.random.default_rng(3)
    x = rng.integers(-2000, 2000, (1, 1024))
    x[0, 10::16] = np.int16(-8)                  # ff f8
    x[0, 11::16] = np.int16(-7)                  # ff f9
    for at, number in ((100, 0), (300, 1), (700, 2)):
        # a header copied from a real frame, CRC-8 and all, but with a number the chain does not expect there
        h = bytearray(F._frame_header(number + 5, False, 256, 44100, 0, 16, True, True))
        h += b"\x00" * (len(h) % 2)
        x[0, at: at + len(h) // 2] = np.frombuffer(bytes(h), dtype=">i2")
    frames = []
    data = F.encode(x, 44100, 16, block_size=256, subframe={"type": "verbatim"}, frames_out=frames,
                    min_frame_in_streaminfo=min_frame_known)
    assert data.count(b"\xff\xf8") > 60
    _check(host, data, frames, 1, 1024)


def test_total_samples_from_the_frames_when_streaminfo_has_none(host):
    frames = []
    data = F.encode(_smooth(1, 700, 4), 44100, 16, block_size=192, frames_out=frames, total_in_streaminfo=False)
    _check(host, data, frames, 1, 700)


def test_zero_frames(host):
    facts, table = host.flac_index(F.encode(np.zeros((2, 0), np.int64), 44100, 16))
    assert len(table) == 0 and facts["total_samples"] == 0 and facts["channels"] == 2


def test_rejections(host):
    from audio_tokens_amd._lib import NativeError
    frames = []
    good = F.encode(_smooth(1, 1000, 5), 44100, 16, block_size=256, frames_out=frames)

    def code(data):
        with pytest.raises(NativeError) as e:
            host.flac_index(data)
        assert "at_flac_index_host" in str(e.value)
        return e.value.code

    assert code(b"RIFF" + good[4:]) == -7                              # no fLaC marker
    assert code(b"") == -7
    assert code(b"OggS" + good) == -8                                  # Ogg encapsulation
    assert code(F.encode(np.zeros((1, 64), np.int64), 44100, 32, block_size=64, subframe={"type": "verbatim"})) == -8
    assert code(good[: frames[-1]["offset"] + 3]) == -9                # the final frame cut off in its header
    assert code(good[: frames[2]["offset"]]) == -9                     # whole frames missing
    assert code(good[:20]) == -9                                       # metadata cut short
    assert len({-7, -8, -9}) == 3
