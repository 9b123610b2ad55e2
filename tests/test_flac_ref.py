"""The test-side FLAC encoder and reference decoder (tests/flac_ref.py) against each other and against values that can
be checked by hand.  CPU only; the product is not involved."""
import hashlib

import numpy as np
import pytest

import flac_ref as F


def _noise(C, L, bps, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    hi = int((1 << (bps - 1)) * scale)
    return rng.integers(-hi, hi, (C, L))


def _smooth(C, L, bps, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    x = np.stack([np.sin(t * (0.01 + 0.003 * c) + c) for c in range(C)]) * (1 << (bps - 2))
    return (x + rng.integers(-4, 5, (C, L))).astype(np.int64)


def test_crc_pins():
    assert F.crc8(b"123456789") == 0xF4          # CRC-8, polynomial 0x07, initial value 0
    assert F.crc16(b"123456789") == 0xFEE8       # CRC-16, polynomial 0x8005, initial value 0, not reflected
    assert F.crc8(b"") == 0 and F.crc16(b"\x00\x00") == 0


def test_zigzag_and_rice_pins():
    assert [F.zigzag(v) for v in (0, -1, 1, -2, 2, -3)] == [0, 1, 2, 3, 4, 5]
    assert F.rice_bits(0, 0) == "1" and F.rice_bits(-1, 0) == "01"
    assert F.rice_bits(5, 2) == "00110"          # zig-zag 10 = 0b10'10: quotient 2 -> "001", remainder "10"
    assert F.rice_bits(-6, 2) == "00111"         # zig-zag 11 = 0b10'11


def test_hand_built_constant_stream():
    # mono, 16 bits, 22 050 Hz, one 16-sample block of the constant 5
    info = bytes.fromhex("0010" "0010" "00000c" "00000c"      # block size 16..16, frame size 12..12
                         "056220f000000010")                  # 22050 (20 bits) | 1 channel | 16 bits | 16 samples (36 bits)
    info += hashlib.md5(b"\x05\x00" * 16).digest()
    frame = bytes.fromhex("fff8" "66" "08" "00" "0f")         # sync, fixed | size code 0110, rate code 0110 | mono, 16 bit |
    frame += bytes.fromhex("e2")                              # frame 0 | block size - 1;  CRC-8 of those six bytes
    frame += bytes.fromhex("00" "0005")                       # subframe: 0, constant 000000, no wasted bits; the value
    frame += bytes.fromhex("5e9b")                            # CRC-16 of the frame
    by_hand = b"fLaC" + bytes.fromhex("80000022") + info + frame
    assert F.crc8(frame[:6]) == 0xE2 and F.crc16(frame[:-2]) == 0x5E9B
    got = F.encode(np.full((1, 16), 5), 22050, 16, block_size=16, subframe={"type": "constant"})
    assert got == by_hand
    x, sr, bps = F.decode(by_hand)
    assert (x == 5).all() and x.shape == (1, 16) and (sr, bps) == (22050, 16)


def _lpc(order, precision, shift, seed=0):
    rng = np.random.default_rng(seed)
    lim = 1 << (precision - 1)
    c = rng.integers(-lim, lim, order)
    return {"type": "lpc", "order": order, "precision": precision, "shift": shift, "coefs": c}


CASES = {
    "mono16_default": dict(x=_smooth(1, 5000, 16, 1), bps=16, kw=dict(block_size=1152)),
    "stereo_mid_side": dict(x=_noise(2, 3000, 16, 2), bps=16, kw=dict(block_size=576, assignment="mid_side")),
    "stereo_left_side": dict(x=_noise(2, 3000, 16, 3), bps=16, kw=dict(block_size=576, assignment="left_side")),
    "stereo_side_right": dict(x=_noise(2, 3000, 16, 4), bps=16, kw=dict(block_size=576, assignment="side_right")),
    "eight_channels_8bit": dict(x=_noise(8, 700, 8, 5), bps=8, kw=dict(block_size=192, subframe={"type": "fixed", "order": 1})),
    "bps12_verbatim": dict(x=_noise(1, 500, 12, 6), bps=12, kw=dict(block_size=255, subframe={"type": "verbatim"})),
    "bps20_fixed4": dict(x=_smooth(1, 2000, 20, 7), bps=20, kw=dict(block_size=257, subframe={"type": "fixed", "order": 4})),
    "bps24_lpc32": dict(x=_noise(1, 1024, 24, 8), bps=24, kw=dict(block_size=512, subframe=_lpc(32, 15, 14))),
    "lpc8_prec12_shift7": dict(x=_smooth(2, 2048, 16, 9), bps=16, kw=dict(block_size=1024, subframe=_lpc(8, 12, 7))),
    "lpc1_prec2_shift0": dict(x=_noise(1, 600, 16, 10, 0.2), bps=16, kw=dict(block_size=300, subframe=_lpc(1, 2, 0))),
    "variable_blocks": dict(x=_smooth(1, 16 + 17 + 4096 + 300, 16, 11), bps=16, kw=dict(block_size=[16, 17, 4096, 300])),
    "method1_param15": dict(x=_noise(1, 512, 24, 12), bps=24,
                            kw=dict(block_size=256, subframe={"type": "fixed", "order": 0, "method": 1, "param": 15})),
    "partitions_max": dict(x=_smooth(1, 1024, 16, 13), bps=16,
                           kw=dict(block_size=256, subframe={"type": "fixed", "order": 2, "partition_order": 7})),
    "escape_widths": dict(x=np.concatenate([np.zeros((1, 64), np.int64), _noise(1, 192, 16, 14)], axis=1), bps=16,
                          kw=dict(block_size=256, subframe={"type": "fixed", "order": 0, "partition_order": 2,
                                                            "escape": (0, 2)})),
    "wasted3": dict(x=_noise(2, 600, 16, 15, 0.1) * 8, bps=16,
                    kw=dict(block_size=300, assignment="mid_side",      # (mid = (l + r) >> 1 keeps two of the three)
                            subframe=lambda f, ch: {"type": "fixed", "order": 1, "wasted": 2 + ch})),
    "bps_from_streaminfo": dict(x=_smooth(1, 400, 16, 16), bps=16, kw=dict(block_size=192, bps_in_header=False,
                                                                          rate_in_header=False)),
    "odd_rate": dict(x=_smooth(1, 400, 16, 17), bps=16, sr=11025, kw=dict(block_size=192)),
    "empty": dict(x=np.zeros((2, 0), np.int64), bps=16, kw=dict(block_size=4096)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_round_trip(name):
    case = CASES[name]
    sr = case.get("sr", 44100)
    frames = []
    data = F.encode(case["x"], sr, case["bps"], frames_out=frames, **case["kw"])
    y, sr_out, bps_out = F.decode(data)
    assert (sr_out, bps_out) == (sr, case["bps"])
    assert y.shape == case["x"].shape and np.array_equal(y, case["x"])
    assert sum(f["block_size"] for f in frames) == case["x"].shape[1]


def test_decoder_rejects_a_flipped_bit():
    data = bytearray(F.encode(_smooth(1, 600, 16, 20), 44100, 16, block_size=192))
    data[-10] ^= 0x10
    with pytest.raises(ValueError):
        F.decode(bytes(data))


def test_encoder_refuses_a_residual_beyond_32_bits():
    x = _noise(1, 64, 24, 21)
    spec = {"type": "lpc", "order": 32, "precision": 15, "shift": 0, "coefs": np.full(32, 16383)}
    with pytest.raises(AssertionError, match="32 bits"):
        F.encode(x, 44100, 24, block_size=64, subframe=spec)
