// logmel_tables.h -- the host-side tables the three log-mel kernels share (logmel.hip: the tuned 512-point kernel;
// logmel_any.hip: the power-of-two and the mixed-radix / Bluestein kernels): periodic Hann window, banded form of a mel
// filterbank, layout of the blob a table slot holds.  Plain C++, no HIP include: tests/host_harness/logmel_tables_host.cpp.
//
//   [head floats, filled by the caller] [start: n_mels ints][len][off][pad to table_ints(n_mels)] [weights ...]
//
// start | len | off | pad | weights is ONE contiguous run of 4-byte words: the tuned kernel copies table_ints(n_mels) + nw
// words starting at `start` into LDS in one loop and finds the weights behind the padded ints there.  The padding keeps
// the weights a multiple of 16 bytes behind `start`; behind a head of a multiple of four floats (the tuned kernel's)
// both are 16-byte aligned in the slot, which that kernel's 16-byte reads of the quad weights need.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

namespace lmt {

// torch.hann_window(n, periodic=True): computed in double, rounded to float
inline void hann_periodic(int n, float* out) {
    for (int i = 0; i < n; i++) out[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / n));
}

// Filter m of fb [nbin][n_mels] as its non-zero band: bins start[m] .. of len[m] groups of `gran` bins, weights at
// wts[off[m] ...].  gran == 1: the band as it is (start = first non-zero tap, len = last - first + 1).  gran == 4: the
// band widened to whole 4-aligned quads of bins (logmel_core.h mel_band reads power and weights 16 bytes at a time),
// zero weights for the padding and for bins >= nbin, len in quads.  A filter with no non-zero tap: start = len = 0.
inline void band_tables(const float* fb, int nbin, int n_mels, int gran, int* start, int* len, int* off,
                        std::vector<float>& wts) {
    wts.clear();
    for (int m = 0; m < n_mels; m++) {
        int lo = nbin, hi = -1;
        for (int f = 0; f < nbin; f++)
            if (fb[(size_t)f * n_mels + m] != 0.0f) { lo = f < lo ? f : lo; hi = f; }
        const int s = hi < 0 ? 0 : (lo / gran) * gran;
        const int e = hi < 0 ? 0 : ((hi + gran) / gran) * gran;
        start[m] = s;
        len[m] = (e - s) / gran;
        off[m] = (int)wts.size();
        for (int f = s; f < e; f++) wts.push_back(f < nbin ? fb[(size_t)f * n_mels + m] : 0.0f);
    }
}

// words the three int tables take, padded to a multiple of four
inline size_t table_ints(int n_mels) { return ((size_t)3 * n_mels + 3) & ~(size_t)3; }

struct BlobLayout { size_t ints, wts; };   // word offsets of `start` (len, off: + n_mels each) and of the weights
inline BlobLayout blob_layout(size_t head_floats, int n_mels) { return {head_floats, head_floats + table_ints(n_mels)}; }

// cuts `blob` behind its first head_floats words (the caller's head) and appends start | len | off | pad | weights;
// ints: the 3 n_mels words of start | len | off
inline void pack_tables(std::vector<float>& blob, size_t head_floats, int n_mels, const int* ints, const std::vector<float>& wts) {
    blob.resize(head_floats);
    blob.resize(head_floats + table_ints(n_mels), 0.0f);   // (the pad words are zero)
    std::memcpy(&blob[head_floats], ints, sizeof(int) * 3 * n_mels);
    blob.insert(blob.end(), wts.begin(), wts.end());
}

// band_tables at `gran`, packed behind the head; returns the number of weights
inline size_t pack_bands(std::vector<float>& blob, size_t head_floats, const float* fb, int nbin, int n_mels, int gran) {
    std::vector<int> ints(3 * (size_t)n_mels);
    std::vector<float> wts;
    band_tables(fb, nbin, n_mels, gran, &ints[0], &ints[n_mels], &ints[2 * (size_t)n_mels], wts);
    pack_tables(blob, head_floats, n_mels, ints.data(), wts);
    return wts.size();
}

}  // namespace lmt
