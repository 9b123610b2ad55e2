// flac_host.cpp -- at_flac_index_host: the host half of the FLAC reader (no GPU work, no context).
//
// Stands in for the container handling of torchaudio.load(path) (processors/spectrogram_generator.py:99 of
// danavery/audio-tokens): finds STREAMINFO and every audio frame of a native FLAC stream, so that flac.hip can decode
// the frames independently, one lane each.  Nothing is decoded here; a frame is recognised by its header alone (sync,
// no reserved code, CRC-8, agreement with STREAMINFO, a coded number that continues the chain).  Format: the FLAC
// format specification (RFC 9639); all fields MSB first.
#include <cstdint>
#include <cstring>

#include "at_internal.h"

namespace {

struct Crc8Table {
    uint8_t t[256];
    Crc8Table() {
        for (int i = 0; i < 256; i++) {
            unsigned c = (unsigned)i;
            for (int b = 0; b < 8; b++) c = (c & 0x80) ? ((c << 1) ^ 0x07) : (c << 1);
            t[i] = (uint8_t)c;
        }
    }
};
const Crc8Table g_crc8;

struct FrameHeader {
    int variable;        // blocking strategy bit
    int block_size;
    int sample_rate;     // 0 = as STREAMINFO
    int channel_assignment;
    int bits_per_sample; // 0 = as STREAMINFO
    int header_bytes;
    uint64_t number;     // frame number (fixed) or first sample number (variable)
};

// p[0..avail) starts at a candidate; true = a complete, self-consistent frame header
bool parse_frame_header(const uint8_t* p, int64_t avail, FrameHeader* h) {
    if (avail < 6 || p[0] != 0xFF || (p[1] & 0xFE) != 0xF8) return false;  // sync 11111111 111110, reserved 0
    h->variable = p[1] & 1;
    const int bs = p[2] >> 4, sr = p[2] & 15, ch = p[3] >> 4, ss = (p[3] >> 1) & 7;
    if ((p[3] & 1) || bs == 0 || sr == 15 || ch > 10 || ss == 3 || ss == 7) return false;  // (32-bit samples: not read)
    // the coded number: UTF-8 extended to 7 bytes
    const uint8_t b0 = p[4];
    int extra;
    uint64_t v;
    if (b0 < 0x80) { extra = 0; v = b0; }
    else if ((b0 & 0xE0) == 0xC0) { extra = 1; v = b0 & 0x1F; }
    else if ((b0 & 0xF0) == 0xE0) { extra = 2; v = b0 & 0x0F; }
    else if ((b0 & 0xF8) == 0xF0) { extra = 3; v = b0 & 0x07; }
    else if ((b0 & 0xFC) == 0xF8) { extra = 4; v = b0 & 0x03; }
    else if ((b0 & 0xFE) == 0xFC) { extra = 5; v = b0 & 0x01; }
    else if (b0 == 0xFE) { extra = 6; v = 0; }
    else return false;
    if (!h->variable && extra == 6) return false;  // a frame number has 31 bits
    int i = 5 + extra;
    const int tail = (bs == 6 ? 1 : bs == 7 ? 2 : 0) + (sr == 12 ? 1 : (sr == 13 || sr == 14) ? 2 : 0);
    if (avail < i + tail + 1) return false;
    for (int j = 0; j < extra; j++) {
        if ((p[5 + j] & 0xC0) != 0x80) return false;
        v = (v << 6) | (p[5 + j] & 0x3F);
    }
    h->number = v;
    if (bs == 1) h->block_size = 192;
    else if (bs <= 5) h->block_size = 576 << (bs - 2);
    else if (bs == 6) { h->block_size = p[i] + 1; i += 1; }
    else if (bs == 7) { h->block_size = ((p[i] << 8) | p[i + 1]) + 1; i += 2; }
    else h->block_size = 256 << (bs - 8);
    static const int kRates[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
    if (sr < 12) h->sample_rate = kRates[sr];
    else if (sr == 12) { h->sample_rate = p[i] * 1000; i += 1; }
    else if (sr == 13) { h->sample_rate = (p[i] << 8) | p[i + 1]; i += 2; }
    else { h->sample_rate = ((p[i] << 8) | p[i + 1]) * 10; i += 2; }
    static const int kBits[8] = {0, 8, 12, 0, 16, 20, 24, 0};
    h->bits_per_sample = kBits[ss];
    h->channel_assignment = ch;
    uint8_t crc = 0;
    for (int j = 0; j < i; j++) crc = g_crc8.t[crc ^ p[j]];
    if (crc != p[i]) return false;
    h->header_bytes = i + 1;
    return true;
}

}  // namespace

extern "C" int at_flac_index_host(const uint8_t* d, int64_t n, at_flac_info* info, at_flac_frame* frames,
                                  int64_t capacity, int64_t* n_frames) {
    AT_REQUIRE(d && n >= 0 && info && n_frames && capacity >= 0 && (frames || capacity == 0),
               "at_flac_index_host: bad arguments");
    std::memset(info, 0, sizeof(*info));
    *n_frames = 0;
    int64_t pos = 0;
    if (n >= 10 && d[0] == 'I' && d[1] == 'D' && d[2] == '3') {  // ID3v2: version (2), flags (1), sync-safe size (4)
        const int64_t size = ((int64_t)(d[6] & 0x7F) << 21) | ((d[7] & 0x7F) << 14) | ((d[8] & 0x7F) << 7) | (d[9] & 0x7F);
        pos = 10 + size + ((d[5] & 0x10) ? 10 : 0);  // (flag bit 4: a 10-byte footer behind the tag)
        if (pos > n) return at_fail(AT_E_FLAC_CORRUPT, "at_flac_index_host: ID3v2 tag of %lld bytes in a file of %lld",
                                    (long long)pos, (long long)n);
    }
    if (n - pos >= 4 && !std::memcmp(d + pos, "OggS", 4))
        return at_fail(AT_E_FLAC_UNSUPPORTED, "at_flac_index_host: Ogg-encapsulated FLAC is not supported");
    if (n - pos < 4 || std::memcmp(d + pos, "fLaC", 4))
        return at_fail(AT_E_FLAC_NOT_FLAC, "at_flac_index_host: not a FLAC stream (no fLaC marker)");
    pos += 4;

    // metadata blocks: last flag (1), type (7), length (24)
    bool have_info = false;
    int64_t si_total = 0;
    int min_frame = 0;
    for (bool last = false; !last;) {
        if (n - pos < 4) return at_fail(AT_E_FLAC_CORRUPT, "at_flac_index_host: metadata cut short");
        last = (d[pos] & 0x80) != 0;
        const int type = d[pos] & 0x7F;
        const int64_t len = ((int64_t)d[pos + 1] << 16) | (d[pos + 2] << 8) | d[pos + 3];
        pos += 4;
        if (n - pos < len) return at_fail(AT_E_FLAC_CORRUPT, "at_flac_index_host: metadata cut short");
        if (type == 0 && !have_info) {
            if (len != 34) return at_fail(AT_E_FLAC_CORRUPT, "at_flac_index_host: STREAMINFO of %lld bytes", (long long)len);
            const uint8_t* s = d + pos;
            info->min_block = (s[0] << 8) | s[1];
            info->max_block = (s[2] << 8) | s[3];
            min_frame = (s[4] << 16) | (s[5] << 8) | s[6];
            info->sample_rate = (s[10] << 12) | (s[11] << 4) | (s[12] >> 4);
            info->channels = ((s[12] >> 1) & 7) + 1;
            info->bits_per_sample = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
            si_total = ((int64_t)(s[13] & 15) << 32) | ((int64_t)s[14] << 24) | (s[15] << 16) | (s[16] << 8) | s[17];
            have_info = true;
        }
        pos += len;
    }
    if (!have_info) return at_fail(AT_E_FLAC_UNSUPPORTED, "at_flac_index_host: no STREAMINFO block");
    if (info->bits_per_sample > 24 || info->bits_per_sample < 4)
        return at_fail(AT_E_FLAC_UNSUPPORTED, "at_flac_index_host: %d bits per sample (4 to 24 are supported)",
                       info->bits_per_sample);

    // the frame table
    int64_t count = 0, samples = 0, prev = -1;
    int variable = -1;
    at_flac_frame* last_rec = nullptr;
    for (int64_t p = pos; p + 6 <= n;) {
        const uint8_t* q = static_cast<const uint8_t*>(std::memchr(d + p, 0xFF, (size_t)(n - p)));
        if (!q) break;
        p = q - d;
        FrameHeader h;
        const bool ok = parse_frame_header(d + p, n - p, &h) &&
                        (variable < 0 || h.variable == variable) &&
                        h.number == (uint64_t)(h.variable ? samples : count) &&
                        (h.sample_rate == 0 || h.sample_rate == info->sample_rate) &&
                        (h.bits_per_sample == 0 || h.bits_per_sample == info->bits_per_sample) &&
                        (h.channel_assignment < 8 ? h.channel_assignment + 1 == info->channels : info->channels == 2) &&
                        h.block_size <= 65535 && (info->max_block == 0 || h.block_size <= info->max_block) &&
                        (prev < 0 || min_frame == 0 || p - prev >= min_frame);
        if (!ok) { p++; continue; }
        if (prev >= 0 && n - prev > INT32_MAX) return at_fail(AT_E_FLAC_CORRUPT, "at_flac_index_host: frame above 2 GiB");
        if (last_rec) last_rec->length = (int32_t)(p - prev);
        last_rec = nullptr;
        if (count < capacity) {
            at_flac_frame* r = last_rec = frames + count;
            std::memset(r, 0, sizeof(*r));
            r->offset = p;
            r->first_sample = samples;
            r->block_size = h.block_size;
            r->channel_assignment = h.channel_assignment;
            r->bits_per_sample = info->bits_per_sample;
            r->header_bytes = h.header_bytes;
            r->channels = info->channels;
        }
        variable = h.variable;
        prev = p;
        samples += h.block_size;
        count++;
        p += h.header_bytes;
    }
    if (prev >= 0 && n - prev > INT32_MAX) return at_fail(AT_E_FLAC_CORRUPT, "at_flac_index_host: frame above 2 GiB");
    if (last_rec) last_rec->length = (int32_t)(n - prev);
    if (si_total != 0 && samples != si_total)
        return at_fail(AT_E_FLAC_CORRUPT, "at_flac_index_host: the frames hold %lld samples, STREAMINFO announces %lld (%s)",
                       (long long)samples, (long long)si_total, samples < si_total ? "file cut short" : "extra frames");
    info->total_samples = samples;
    info->variable_blocksize = variable > 0 ? 1 : 0;
    const int64_t written = count < capacity ? count : capacity;
    for (int64_t i = 0; i < written; i++) frames[i].out_stride = samples;
    *n_frames = count;
    return AT_OK;
}
