"""Test-side FLAC: an encoder that lets a test choose every coding decision, and a scalar reference decoder.

Both are written from the format description (RFC 9639) in pure Python / numpy, separately from each other and from
the product; they share only the BitWriter / BitReader pair.  There is no libFLAC on the
build machine, so these two pin the product's reading of the format ("parity unpinned against libFLAC").

encode(samples int [C, L], sr, bps, ...) -> bytes
    block_size   int (fixed-blocksize stream) or a list of sizes (variable-blocksize stream; must add up to L)
    assignment   None = independent channels, or "left_side" / "side_right" / "mid_side" (C == 2); or a callable
                 frame index -> one of those
    subframe     a dict, or a callable (frame index, channel) -> dict, with
                   type "constant" | "verbatim" | "fixed" | "lpc";  order;  precision, shift, coefs (lpc);
                   method 0 | 1;  partition_order;  param: None (fitted per partition) | int | list per partition;
                   escape: iterable of partition numbers coded raw;  escape_width: None (smallest that fits) | int;
                   wasted: number of wasted bits (the samples must be multiples of 2^wasted)
    bps_in_header / rate_in_header   False = code 000 / 0000 ("from STREAMINFO") in the frame headers
    frames_out   a list that receives one dict per frame: offset, length, first_sample, block_size
decode(bytes) -> (int32 [C, L], sr, bps), checking CRC-8, CRC-16 and STREAMINFO's MD5.
"""
import hashlib

import numpy as np

# ---- shared: bits and CRCs ---------------------------------------------------------------------------------------


class BitWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def write(self, value, nbits):
        if nbits == 0:
            return
        self.acc = (self.acc << nbits) | (int(value) & ((1 << nbits) - 1))
        self.n += nbits
        if self.n >= 512:
            self._flush()

    def _flush(self):
        k = self.n // 8
        if k:
            rest = self.n - 8 * k
            self.buf += (self.acc >> rest).to_bytes(k, "big")
            self.acc &= (1 << rest) - 1
            self.n = rest

    def align(self):
        if self.n % 8:
            self.write(0, 8 - self.n % 8)

    def bytes(self):
        assert self.n % 8 == 0
        self._flush()
        return bytes(self.buf)


class BitReader:
    def __init__(self, data, pos=0):
        self.data = data
        self.bit = pos * 8

    def read(self, nbits):
        if nbits == 0:
            return 0
        b0, b1 = self.bit // 8, (self.bit + nbits + 7) // 8
        if b1 > len(self.data):
            raise ValueError("read past the end")
        v = int.from_bytes(self.data[b0:b1], "big")
        v = (v >> (b1 * 8 - self.bit - nbits)) & ((1 << nbits) - 1)
        self.bit += nbits
        return v

    def read_signed(self, nbits):
        v = self.read(nbits)
        return v - (1 << nbits) if nbits and v >> (nbits - 1) else v

    def read_unary(self):
        q = 0
        while self.read(1) == 0:
            q += 1
        return q


def crc8(data):
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_CRC16 = []
for _i in range(256):
    _c = _i << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC16.append(_c)


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


def zigzag(r):
    return (r << 1) if r >= 0 else ((-r) << 1) - 1


def rice_bits(r, k):
    """The Rice code of r at parameter k as a string of '0' / '1'."""
    u = zigzag(r)
    return "0" * (u >> k) + "1" + (format(u & ((1 << k) - 1), f"0{k}b") if k else "")


# ---- encoder -----------------------------------------------------------------------------------------------------

_RATES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
_BITS = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}
_FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
_ASSIGN = {"left_side": 8, "side_right": 9, "mid_side": 10}


def _utf8(v):
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1):       # n bytes carry 5n + 1 bits (7 bytes: 36)
        n += 1
    out = [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 1)][::-1]
    lead = (0xFF << (8 - n)) & 0xFF
    return bytes([lead | (v >> (6 * (n - 1)))] + out)


def _min_width(values):
    """Smallest two's complement width holding every value (0 for all zeros)."""
    if values.size == 0 or not values.any():
        return 0
    lo, hi, w = int(values.min()), int(values.max()), 1
    while lo < -(1 << (w - 1)) or hi > (1 << (w - 1)) - 1:
        w += 1
    return w


def _write_subframe(w, s, width, spec):
    """s: int64 [n] samples of one channel of one frame, `width` bits wide."""
    n = len(s)
    kind = spec.get("type", "fixed")
    wasted = int(spec.get("wasted", 0))
    if wasted:
        assert not (s & ((1 << wasted) - 1)).any(), "samples are not multiples of 2^wasted"
        s = s >> wasted
        width -= wasted
    assert width >= 1 and s.min() >= -(1 << (width - 1)) and s.max() < (1 << (width - 1)), "sample out of range"
    order = int(spec.get("order", 0))
    code = {"constant": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 32 + order - 1}[kind]
    w.write(0, 1)
    w.write(code, 6)
    if wasted:
        w.write(1, 1)
        w.write(1, wasted)               # wasted - 1 zeros and a one
    else:
        w.write(0, 1)
    if kind == "constant":
        assert (s == s[0]).all()
        w.write(int(s[0]), width)
        return
    if kind == "verbatim":
        for v in s.tolist():
            w.write(v, width)
        return
    assert order <= n
    if kind == "fixed":
        assert 0 <= order <= 4
        coefs, shift = _FIXED[order], 0
    else:
        assert 1 <= order <= 32
        coefs, shift, prec = [int(c) for c in spec["coefs"]], int(spec["shift"]), int(spec["precision"])
        assert len(coefs) == order and 1 <= prec <= 15 and 0 <= shift <= 15
        assert all(-(1 << (prec - 1)) <= c < (1 << (prec - 1)) for c in coefs)
    for v in s[:order].tolist():
        w.write(v, width)
    if kind == "lpc":
        w.write(prec - 1, 4)
        w.write(shift, 5)
        for c in coefs:
            w.write(c, prec)
    pred = np.zeros(n - order, np.int64)
    for j, c in enumerate(coefs):
        pred += c * s[order - 1 - j: n - 1 - j]
    res = s[order:] - (pred >> shift)
    assert res.size == 0 or (res.min() >= -(1 << 31) and res.max() < (1 << 31)), "residual does not fit 32 bits"
    method = int(spec.get("method", 0))
    pbits, esc = (5, 31) if method else (4, 15)
    porder = int(spec.get("partition_order", 0))
    assert n % (1 << porder) == 0 and (n >> porder) >= order, "partition order not allowed for this block"
    w.write(method, 2)
    w.write(porder, 4)
    params = spec.get("param")
    escapes = set(spec.get("escape", ()))
    at = 0
    for p in range(1 << porder):
        cnt = (n >> porder) - (order if p == 0 else 0)
        r = res[at: at + cnt]
        at += cnt
        if p in escapes:
            ew = spec.get("escape_width")
            ew = _min_width(r) if ew is None else int(ew)
            assert ew >= _min_width(r), "escape width too small"
            w.write(esc, pbits)
            w.write(ew, 5)
            for v in r.tolist():
                w.write(v, ew)
            continue
        u = (r << 1) ^ (r >> 63)
        if params is None:
            k = int(np.argmin([int((u >> kk).sum()) + cnt * (1 + kk) for kk in range(esc)])) if cnt else 0
        else:
            k = int(params if np.isscalar(params) else params[p])
        assert 0 <= k < esc
        w.write(k, pbits)
        mask = (1 << k) - 1
        for uu in u.tolist():
            w.write(1, (uu >> k) + 1)
            w.write(uu & mask, k)


def _frame_header(number, variable, bs, sr, assign_code, bps, bps_in_header, rate_in_header):
    w = BitWriter()
    w.write(0b11111111111110, 14)
    w.write(0, 1)
    w.write(1 if variable else 0, 1)
    if bs == 192:
        bcode = 1
    elif bs in (576, 1152, 2304, 4608):
        bcode = 2 + (576, 1152, 2304, 4608).index(bs)
    elif bs in [256 << i for i in range(8)]:
        bcode = 8 + [256 << i for i in range(8)].index(bs)
    else:
        bcode = 6 if bs <= 256 else 7
    if not rate_in_header:
        rcode = 0
    elif sr in _RATES:
        rcode = _RATES[sr]
    elif sr % 1000 == 0 and sr < 256000:
        rcode = 12
    elif sr < 65536:
        rcode = 13
    else:
        assert sr % 10 == 0 and sr < 655360
        rcode = 14
    w.write(bcode, 4)
    w.write(rcode, 4)
    w.write(assign_code, 4)
    w.write(_BITS[bps] if bps_in_header and bps in _BITS else 0, 3)
    w.write(0, 1)
    for b in _utf8(number):
        w.write(b, 8)
    if bcode == 6:
        w.write(bs - 1, 8)
    elif bcode == 7:
        w.write(bs - 1, 16)
    if rcode == 12:
        w.write(sr // 1000, 8)
    elif rcode == 13:
        w.write(sr, 16)
    elif rcode == 14:
        w.write(sr // 10, 16)
    h = w.bytes()
    return h + bytes([crc8(h)])


def streaminfo(min_bs, max_bs, min_fs, max_fs, sr, channels, bps, total, md5):
    w = BitWriter()
    for v, n in ((min_bs, 16), (max_bs, 16), (min_fs, 24), (max_fs, 24), (sr, 20), (channels - 1, 3), (bps - 1, 5), (total, 36)):
        w.write(v, n)
    return w.bytes() + md5


def metadata_block(kind, payload, last):
    return bytes([(0x80 if last else 0) | kind]) + len(payload).to_bytes(3, "big") + payload


def samples_md5(x, bps):
    """MD5 of the samples interleaved, little-endian, in ceil(bps / 8) bytes each (sign extended)."""
    nb = (bps + 7) // 8
    inter = np.ascontiguousarray(np.asarray(x, np.int64).T).reshape(-1)
    raw = inter.astype("<i8").view(np.uint8).reshape(-1, 8)[:, :nb]
    return hashlib.md5(np.ascontiguousarray(raw).tobytes()).digest()


def encode(samples, sr, bps, block_size=4096, assignment=None, subframe=None, bps_in_header=True, rate_in_header=True,
           frames_out=None, extra_metadata=(), prefix=b"", suffix=b"", total_in_streaminfo=True, min_frame_in_streaminfo=True):
    x = np.atleast_2d(np.asarray(samples)).astype(np.int64)
    C, L = x.shape
    assert 1 <= C <= 8 and 4 <= bps <= 32
    assert L == 0 or (x.min() >= -(1 << (bps - 1)) and x.max() < (1 << (bps - 1)))
    variable = not np.isscalar(block_size)
    sizes = list(block_size) if variable else [block_size] * (L // block_size) + ([L % block_size] if L % block_size else [])
    assert sum(sizes) == L and all(1 <= b <= 65535 for b in sizes)
    frames, at = [], 0
    for fi, bs in enumerate(sizes):
        a = assignment(fi) if callable(assignment) else assignment
        blk = x[:, at: at + bs]
        if a is None:
            chans, widths, acode = list(blk), [bps] * C, C - 1
        else:
            assert C == 2
            left, right = blk
            side = left - right
            chans, widths = {"left_side": ([left, side], [bps, bps + 1]), "side_right": ([side, right], [bps + 1, bps]),
                             "mid_side": ([(left + right) >> 1, side], [bps, bps + 1])}[a]
            acode = _ASSIGN[a]
        w = BitWriter()
        for b in _frame_header(at if variable else fi, variable, bs, sr, acode, bps, bps_in_header, rate_in_header):
            w.write(b, 8)
        for ch, (s, width) in enumerate(zip(chans, widths)):
            spec = subframe(fi, ch) if callable(subframe) else (subframe or {"type": "fixed", "order": min(2, bs)})
            _write_subframe(w, s, width, spec)
        w.align()
        body = w.bytes()
        frames.append(body + crc16(body).to_bytes(2, "big"))
        at += bs
    lens = [len(f) for f in frames]
    info = streaminfo(min(sizes, default=16) if variable else block_size, max(sizes, default=16) if variable else block_size,
                      min(lens, default=0) if min_frame_in_streaminfo else 0, max(lens, default=0), sr, C, bps,
                      L if total_in_streaminfo else 0, samples_md5(x, bps))
    blocks = [(0, info)] + list(extra_metadata)
    head = prefix + b"fLaC" + b"".join(metadata_block(k, p, i == len(blocks) - 1) for i, (k, p) in enumerate(blocks))
    if frames_out is not None:
        off, first = len(head), 0
        for f, bs in zip(frames, sizes):
            frames_out.append({"offset": off, "length": len(f), "first_sample": first, "block_size": bs})
            off += len(f)
            first += bs
    return head + b"".join(frames) + suffix


# ---- reference decoder (scalar, written on its own) -----------------------------------------------------------------

_BLOCK_SIZES = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, **{8 + i: 256 << i for i in range(8)}}
_RATE_CODES = {v: k for k, v in _RATES.items()}
_BIT_CODES = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}


def _crc_bitwise(data, poly, width):
    """MSB-first CRC with initial value 0, one bit at a time (the decoder's own, apart from crc8 / crc16 above)."""
    top, mask, c = 1 << (width - 1), (1 << width) - 1, 0
    for b in data:
        c ^= b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
    return c


def _decode_residual(r, n, order):
    method = r.read(2)
    if method > 1:
        raise ValueError("reserved residual method")
    pbits = 5 if method else 4
    porder = r.read(4)
    if n % (1 << porder) or (n >> porder) < order:
        raise ValueError("partition order not allowed")
    out = []
    for p in range(1 << porder):
        cnt = (n >> porder) - (order if p == 0 else 0)
        k = r.read(pbits)
        if k == (1 << pbits) - 1:
            ew = r.read(5)
            out += [r.read_signed(ew) for _ in range(cnt)]
        else:
            for _ in range(cnt):
                u = (r.read_unary() << k) | r.read(k)
                out.append((u >> 1) ^ -(u & 1))
    return out


def _decode_subframe(r, n, width):
    if r.read(1):
        raise ValueError("subframe padding bit")
    t = r.read(6)
    wasted = 0
    if r.read(1):
        wasted = r.read_unary() + 1
        if wasted >= width:
            raise ValueError("wasted bits")
    width -= wasted
    if t == 0:
        s = [r.read_signed(width)] * n
    elif t == 1:
        s = [r.read_signed(width) for _ in range(n)]
    elif 8 <= t <= 12 or t >= 32:
        order = t - 8 if t < 32 else t - 31
        if order > n:
            raise ValueError("order above block size")
        s = [r.read_signed(width) for _ in range(order)]
        if t >= 32:
            prec = r.read(4) + 1
            if prec == 16:
                raise ValueError("reserved precision")
            shift = r.read_signed(5)
            if shift < 0:
                raise ValueError("negative shift")
            coefs = [r.read_signed(prec) for _ in range(order)]
        else:
            coefs, shift = [[], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1]][order], 0
        for res in _decode_residual(r, n, order):
            acc = 0
            for j in range(order):
                acc += coefs[j] * s[-1 - j]
            s.append(res + (acc >> shift))
    else:
        raise ValueError("reserved subframe type")
    return [v << wasted for v in s]


def decode(data):
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise ValueError("no fLaC marker")
    pos, si = 4, None
    while True:
        last, kind, ln = data[pos] >> 7, data[pos] & 0x7F, int.from_bytes(data[pos + 1: pos + 4], "big")
        if kind == 0:
            si = data[pos + 4: pos + 4 + ln]
        pos += 4 + ln
        if last:
            break
    r = BitReader(si)
    r.read(16), r.read(16), r.read(24), r.read(24)
    sr, C, bps, total, md5 = r.read(20), r.read(3) + 1, r.read(5) + 1, r.read(36), si[18:34]
    chans = [[] for _ in range(C)]
    done = nframes = 0
    while done < total or (total == 0 and pos < len(data)):
        start = pos
        r = BitReader(data, pos)
        if r.read(15) != 0x7FFC:
            raise ValueError("lost sync")
        variable, bcode, rcode, acode, scode = r.read(1), r.read(4), r.read(4), r.read(4), r.read(3)
        if r.read(1) or bcode == 0 or rcode == 15 or acode > 10 or scode == 3:
            raise ValueError("reserved header code")
        lead = r.read(8)
        nbytes = 0
        while lead & (0x80 >> nbytes):
            nbytes += 1
        number = lead & (0x7F >> nbytes) if nbytes else lead
        for _ in range(max(nbytes - 1, 0)):
            number = (number << 6) | (r.read(8) & 0x3F)
        n = r.read(8) + 1 if bcode == 6 else r.read(16) + 1 if bcode == 7 else _BLOCK_SIZES[bcode]
        rate = r.read(8) * 1000 if rcode == 12 else r.read(16) if rcode == 13 else r.read(16) * 10 if rcode == 14 else \
            _RATE_CODES.get(rcode, sr)
        if rate != sr or (scode and _BIT_CODES[scode] != bps):
            raise ValueError("header disagrees with STREAMINFO")
        hend = r.bit // 8
        if _crc_bitwise(data[start:hend], 0x07, 8) != data[hend]:
            raise ValueError("CRC-8 mismatch")
        r.read(8)
        if number != (done if variable else nframes):
            raise ValueError("frame chain broken")
        nframes += 1
        nch = acode + 1 if acode < 8 else 2
        side = {8: 1, 9: 0, 10: 1}.get(acode)
        sub = [_decode_subframe(r, n, bps + (1 if ch == side else 0)) for ch in range(nch)]
        if acode == 8:
            sub[1] = [a - b for a, b in zip(sub[0], sub[1])]
        elif acode == 9:
            sub[0] = [a + b for a, b in zip(sub[0], sub[1])]
        elif acode == 10:
            mid = [(m << 1) | (s & 1) for m, s in zip(sub[0], sub[1])]
            sub = [[(m + s) >> 1 for m, s in zip(mid, sub[1])], [(m - s) >> 1 for m, s in zip(mid, sub[1])]]
        r.read((8 - r.bit % 8) % 8)
        end = r.bit // 8
        if _crc_bitwise(data[start:end], 0x8005, 16) != r.read(16):
            raise ValueError("CRC-16 mismatch")
        pos = end + 2
        for ch in range(C):
            chans[ch] += sub[ch]
        done += n
    out = np.array(chans, dtype=np.int64).reshape(C, -1)
    nb = (bps + 7) // 8
    raw = b"".join(int(v).to_bytes(nb, "little", signed=True) for v in out.T.reshape(-1))
    if hashlib.md5(raw).digest() != md5:
        raise ValueError("MD5 mismatch")
    return out.astype(np.int32), sr, bps
