// flac.hip -- at_flac_decode_f32: the audio frames of a batch of FLAC files decoded on gfx950, one lane per frame.
//
// Stands in for the codec half of torchaudio.load(path) (processors/spectrogram_generator.py:99 of
// danavery/audio-tokens).  at_flac_index_host (flac_host.cpp) has found the frames; a frame depends on no other frame,
// so a batch of 5000 ten-second clips is ~0.5 M independent pieces of work.  Inside a frame everything is serial:
// the subframes follow one another in the bit stream, a Rice code's position depends on every code before it and a
// predicted sample on the samples before it.  So: one lane = one frame, 64 frames per wave, one wave per workgroup.
//
// Layout of a lane's work
//   * bit reader: a 64-bit window refilled with aligned 32-bit words of the byte buffer; words past the frame's own
//     bytes read as zero and the overrun shows in the count of consumed bits;
//   * predictor: the fixed predictors are LPC with the binomial coefficients and shift 0, so there is one restore loop;
//     coefficients and the ring of the last 32 samples live in LDS, [j][lane] (conflict free), sums are 64-bit;
//   * stores: a lane writes its own run of each channel row.  Independent channels are stored as floats right away;
//     a decorrelated stereo pair is stored as integers in the output rows themselves (a float slot holds an int32) and
//     turned into left / right floats by a second loop of the same lane -- no scratch buffer;
//   * CRC-16 (x^16 + x^15 + x^2 + 1, initial value 0) over the frame's bytes from a 256-entry LDS table.
//
// Safety (the files come from disk): every trip count is a field of the frame record or is clamped by one -- block
// size, channels, predictor order <= block size, partition sizes, unary runs end with the frame's bits -- and the
// record itself is checked against the buffer sizes before anything is read.  A malformed frame ends in a status.
#include "at_internal.h"

namespace {

constexpr int WG = 64;

struct BitReader {
    const uint32_t* words;  // the byte buffer as big-endian words
    long next, last;        // next word to load; last word that overlaps the frame's bytes
    uint64_t acc;           // the next `cnt` bits of the stream, left-justified; the bits below them are zero
    int cnt;
    long used;              // bits consumed since the frame's sync code

    __device__ __forceinline__ void refill() {  // cnt < 32 on entry
        uint32_t w = 0;
        if (next <= last) w = __builtin_bswap32(words[next]);
        next++;
        acc |= (uint64_t)w << (32 - cnt);
        cnt += 32;
    }
    __device__ __forceinline__ uint32_t get(int n) {  // 0 <= n <= 32
        if (cnt < n) refill();
        const uint32_t v = n ? (uint32_t)(acc >> (64 - n)) : 0u;
        acc <<= n;
        cnt -= n;
        used += n;
        return v;
    }
    __device__ __forceinline__ int32_t gets(int n) {  // two's complement, 0 <= n <= 32 (width 0 reads as 0)
        if (n == 0) return 0;
        return (int32_t)(get(n) << (32 - n)) >> (32 - n);
    }
    // number of zero bits in front of the next one bit, which is consumed too; gives up once `limit` bits are used
    __device__ __forceinline__ uint32_t unary(long limit) {
        uint32_t q = 0;
        for (;;) {
            if (cnt == 0) refill();
            const int z = acc ? __builtin_clzll(acc) : 64;
            if (z < cnt) {
                acc <<= (z + 1);
                cnt -= z + 1;
                used += z + 1;
                return q + (uint32_t)z;
            }
            q += (uint32_t)cnt;
            used += cnt;
            acc = 0;
            cnt = 0;
            if (used > limit) return q;
        }
    }
};

__device__ __forceinline__ unsigned crc16_step(const unsigned short* tab, unsigned crc, unsigned byte) {
    return ((crc << 8) ^ tab[((crc >> 8) ^ byte) & 255u]) & 0xFFFFu;
}

// one frame; returns AT_FLAC_*
__device__ int decode_frame(const uint8_t* __restrict__ data, long data_bytes, const at_flac_frame& fr,
                            float* __restrict__ out, long out_floats, int (*coef)[WG], int (*hist)[WG],
                            const unsigned short* crc_tab) {
    const int lane = threadIdx.x;
    const int bs = fr.block_size, nch = fr.channels, bps = fr.bits_per_sample, ca = fr.channel_assignment;
    // the record against the buffers: nothing below reads or writes outside what these lines allow
    if (nch < 1 || nch > 8 || bps < 4 || bps > 24 || bs < 1 || bs > 65535 || ca < 0 || ca > 10 ||
        (ca < 8 ? nch != ca + 1 : nch != 2) || fr.header_bytes < 6 || fr.header_bytes > 16 ||
        fr.length < fr.header_bytes || fr.offset < 0 || fr.offset > data_bytes || fr.length > data_bytes - fr.offset ||
        fr.first_sample < 0 || fr.out_stride < 0 || fr.first_sample > fr.out_stride - bs || fr.out_base < 0 ||
        fr.out_base > out_floats || fr.out_stride > (out_floats - fr.out_base) / nch)
        return AT_FLAC_BAD_RECORD;

    const long limit = (long)fr.length * 8;  // bits of the frame
    BitReader rd;
    rd.words = reinterpret_cast<const uint32_t*>(data);
    const long start = fr.offset + fr.header_bytes;  // the header was parsed, and its CRC-8 checked, by the indexer
    rd.next = start >> 2;
    rd.last = (fr.offset + fr.length + 3) >> 2;      // < (data_bytes + 8) / 4: inside the caller's padding
    rd.acc = 0;
    rd.cnt = 0;
    rd.used = 0;
    rd.get((int)(start & 3) * 8);
    rd.used = (long)fr.header_bytes * 8;

    float* const base = out + fr.out_base + fr.first_sample;
    const float scale = __builtin_ldexpf(1.0f, 1 - bps);  // 1 / 2^(bps-1)
    const bool pair = ca >= 8;

    for (int ch = 0; ch < nch; ch++) {
        float* const row = base + (long)ch * fr.out_stride;
        int* const irow = reinterpret_cast<int*>(row);
        int width = bps + (((ca == 8 || ca == 10) && ch == 1) || (ca == 9 && ch == 0) ? 1 : 0);  // the side channel
        if (rd.get(1)) return AT_FLAC_BAD_SUBFRAME;
        const int type = (int)rd.get(6);
        int wasted = 0;
        if (rd.get(1)) {
            const uint32_t zeros = rd.unary(limit);  // k - 1 zeros and a one: k wasted bits
            if (zeros >= (uint32_t)(width - 1)) return rd.used > limit ? AT_FLAC_OVERRUN : AT_FLAC_BAD_SUBFRAME;
            wasted = (int)zeros + 1;
        }
        width -= wasted;
#define AT_FLAC_STORE(i, s)                                                    \
    do {                                                                       \
        const int v_ = (int)((unsigned)(s) << wasted);                         \
        if (pair) irow[i] = v_; else row[i] = (float)v_ * scale;               \
    } while (0)
        if (type == 0) {  // constant
            const int s = rd.gets(width);
            for (int i = 0; i < bs; i++) AT_FLAC_STORE(i, s);
        } else if (type == 1) {  // verbatim
            for (int i = 0; i < bs; i++) {
                const int s = rd.gets(width);
                AT_FLAC_STORE(i, s);
            }
        } else {
            int order, shift = 0;
            const bool lpc = type >= 32;
            if (lpc) order = type - 31;
            else if (type >= 8 && type <= 12) order = type - 8;
            else return AT_FLAC_BAD_SUBFRAME;
            if (order > bs) return AT_FLAC_BAD_SUBFRAME;
            for (int i = 0; i < order; i++) {  // warm-up samples
                const int s = rd.gets(width);
                hist[i & 31][lane] = s;
                AT_FLAC_STORE(i, s);
            }
            if (lpc) {
                const int prec = (int)rd.get(4) + 1;
                if (prec == 16) return AT_FLAC_RESERVED;
                shift = rd.gets(5);
                if (shift < 0) return AT_FLAC_RESERVED;
                for (int j = 0; j < order; j++) coef[j][lane] = rd.gets(prec);
            } else {  // s(-1), 2s(-1) - s(-2), 3s(-1) - 3s(-2) + s(-3), 4s(-1) - 6s(-2) + 4s(-3) - s(-4)
                const int c1 = order, c2 = -(order * (order - 1)) / 2, c3 = order == 3 ? 1 : 4, c4 = -1;
                if (order >= 1) coef[0][lane] = c1;
                if (order >= 2) coef[1][lane] = c2;
                if (order >= 3) coef[2][lane] = c3;
                if (order >= 4) coef[3][lane] = c4;
            }
            // residual
            const unsigned method = rd.get(2);
            if (method >= 2) return AT_FLAC_RESERVED;
            const int pbits = method ? 5 : 4, esc = method ? 31 : 15;
            const int porder = (int)rd.get(4);
            if ((bs & ((1 << porder) - 1)) || (bs >> porder) < order) return AT_FLAC_RESERVED;
            const int psize = bs >> porder;
            int i = order;
            for (int part = 0; part < (1 << porder); part++) {
                const int n = psize - (part == 0 ? order : 0);
                const int k = (int)rd.get(pbits);
                const int ew = k == esc ? (int)rd.get(5) : -1;  // escaped partition: raw samples of ew bits
                for (int t = 0; t < n; t++, i++) {
                    int r;
                    if (ew >= 0) {
                        r = rd.gets(ew);
                    } else {
                        const uint32_t q = rd.unary(limit);
                        const uint32_t u = (q << k) | rd.get(k);
                        r = (int)((u >> 1) ^ (0u - (u & 1u)));
                    }
                    long sum = 0;
                    for (int j = 0; j < order; j++) sum += (long)coef[j][lane] * (long)hist[(i - 1 - j) & 31][lane];
                    const int s = (int)((unsigned)r + (unsigned)(int)(sum >> shift));
                    hist[i & 31][lane] = s;
                    AT_FLAC_STORE(i, s);
                }
                if (rd.used > limit) return AT_FLAC_OVERRUN;
            }
        }
#undef AT_FLAC_STORE
        if (rd.used > limit) return AT_FLAC_OVERRUN;
    }

    if (pair) {  // the pair's rows hold integers: left / right from them, in place (float bits through the int rows)
        int* const i0 = reinterpret_cast<int*>(base);
        int* const i1 = reinterpret_cast<int*>(base + fr.out_stride);
        for (int i = 0; i < bs; i++) {
            const int a = i0[i], b = i1[i];
            int l, r;
            if (ca == 8) { l = a; r = (int)((unsigned)a - (unsigned)b); }          // left, side
            else if (ca == 9) { r = b; l = (int)((unsigned)a + (unsigned)b); }     // side, right
            else {                                                                  // mid, side
                const int m = (int)(((unsigned)a << 1) | ((unsigned)b & 1u));
                l = (int)((unsigned)m + (unsigned)b) >> 1;
                r = (int)((unsigned)m - (unsigned)b) >> 1;
            }
            i0[i] = __float_as_int((float)l * scale);
            i1[i] = __float_as_int((float)r * scale);
        }
    }

    rd.get((int)((8 - (rd.used & 7)) & 7));  // zero padding to the byte boundary
    const long nbytes = rd.used >> 3;
    const unsigned want = rd.get(16);
    if (rd.used > limit) return AT_FLAC_OVERRUN;
    unsigned crc = 0;
    long a = fr.offset;
    const long e = fr.offset + nbytes;
    for (; a < e && (a & 3); a++) crc = crc16_step(crc_tab, crc, data[a]);
    for (; a + 4 <= e; a += 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(data + a);
        crc = crc16_step(crc_tab, crc, w & 255u);
        crc = crc16_step(crc_tab, crc, (w >> 8) & 255u);
        crc = crc16_step(crc_tab, crc, (w >> 16) & 255u);
        crc = crc16_step(crc_tab, crc, w >> 24);
    }
    for (; a < e; a++) crc = crc16_step(crc_tab, crc, data[a]);
    return crc == want ? AT_FLAC_OK : AT_FLAC_CRC16;
}

__global__ void __launch_bounds__(WG) flac_decode_kernel(const uint8_t* __restrict__ data, long data_bytes,
                                                         const at_flac_frame* __restrict__ frames, long n_frames,
                                                         int n_clips, float* __restrict__ out, long out_floats,
                                                         int* __restrict__ frame_status, unsigned* __restrict__ clip_key) {
    __shared__ int coef[32][WG];
    __shared__ int hist[32][WG];
    __shared__ unsigned short crc_tab[256];
    for (int i = threadIdx.x; i < 256; i += WG) {
        unsigned c = (unsigned)i << 8;
        for (int b = 0; b < 8; b++) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) : (c << 1);
        crc_tab[i] = (unsigned short)c;
    }
    __syncthreads();
    const long f = (long)blockIdx.x * WG + threadIdx.x;
    if (f >= n_frames) return;
    const at_flac_frame fr = frames[f];
    const int st = decode_frame(data, data_bytes, fr, out, out_floats, coef, hist, crc_tab);
    frame_status[f] = st;
    // a clip reports its first failing frame: the lowest (frame index, kind) key wins
    if (st != AT_FLAC_OK && fr.clip >= 0 && fr.clip < n_clips) atomicMin(&clip_key[fr.clip], ((unsigned)f << 3) | (unsigned)st);
}

__global__ void __launch_bounds__(256) flac_clip_status_kernel(int* __restrict__ clip_status, int n_clips) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_clips) return;
    const unsigned key = (unsigned)clip_status[c];
    clip_status[c] = key == 0xFFFFFFFFu ? AT_FLAC_OK : (int)(key & 7u);
}

}  // namespace

extern "C" int at_flac_decode_f32(const uint8_t* data, int64_t data_bytes, const at_flac_frame* frames, int64_t n_frames,
                                  int32_t n_clips, float* out, int64_t out_floats, int32_t* frame_status,
                                  int32_t* clip_status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(n_frames >= 0 && n_frames < (1LL << 28) && n_clips >= 0 && data_bytes >= 0 && out_floats >= 0,
               "at_flac_decode_f32: bad sizes");
    if (n_clips > 0) {
        AT_REQUIRE(clip_status, "at_flac_decode_f32: clip_status is null");
        AT_HIP(hipMemsetAsync(clip_status, 0xFF, sizeof(int32_t) * (size_t)n_clips, stream));
    }
    if (n_frames > 0) {
        AT_REQUIRE(data && frames && frame_status && (out || out_floats == 0), "at_flac_decode_f32: null buffer");
        AT_REQUIRE((reinterpret_cast<uintptr_t>(data) & 3u) == 0 && (reinterpret_cast<uintptr_t>(frames) & 7u) == 0,
                   "at_flac_decode_f32: data must be 4-byte aligned, frames 8-byte aligned");
        AT_LAUNCH(flac_decode_kernel, dim3((unsigned)((n_frames + WG - 1) / WG)), dim3(WG), 0, stream, data,
                  (long)data_bytes, frames, (long)n_frames, (int)n_clips, out, (long)out_floats, frame_status,
                  reinterpret_cast<unsigned*>(clip_status));
    }
    if (n_clips > 0)
        AT_LAUNCH(flac_clip_status_kernel, dim3((unsigned)((n_clips + 255) / 256)), dim3(256), 0, stream, clip_status,
                  (int)n_clips);
    return AT_OK;
}
