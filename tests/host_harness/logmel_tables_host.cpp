// logmel_tables_host.cpp -- the host-side table builders of audio_tokens_amd/csrc/logmel_tables.h behind a C interface.
// TEST INFRASTRUCTURE (built on the fly by tests/test_logmel_tables_host.py with g++).
#include <cstring>
#include <vector>

#include "../../audio_tokens_amd/csrc/logmel_tables.h"

extern "C" void lmt_host_hann(int n, float* out) { lmt::hann_periodic(n, out); }

// start / len / off: [n_mels]; wts: room for wts_cap floats.  Returns the number of weights (nothing is written to wts
// when they do not fit).
extern "C" long lmt_host_bands(const float* fb, int nbin, int n_mels, int gran, int* start, int* len, int* off, float* wts,
                               long wts_cap) {
    std::vector<float> w;
    lmt::band_tables(fb, nbin, n_mels, gran, start, len, off, w);
    if ((long)w.size() <= wts_cap && !w.empty()) std::memcpy(wts, w.data(), w.size() * sizeof(float));
    return (long)w.size();
}

extern "C" void lmt_host_layout(long head_floats, int n_mels, long* ints, long* wts, long* nint) {
    const lmt::BlobLayout lay = lmt::blob_layout((size_t)head_floats, n_mels);
    *ints = (long)lay.ints;
    *wts = (long)lay.wts;
    *nint = (long)lmt::table_ints(n_mels);
}

// The blob pack_bands leaves behind a head of head_floats copies of `head_value`, packed twice (gran 4, then `gran`) the
// way the tuned path retries; returns its length in words (nothing is written when it exceeds blob_cap).
extern "C" long lmt_host_pack(const float* fb, int nbin, int n_mels, int gran, long head_floats, float head_value, float* blob,
                              long blob_cap, long* n_wts) {
    std::vector<float> b((size_t)head_floats, head_value);
    lmt::pack_bands(b, (size_t)head_floats, fb, nbin, n_mels, 4);
    *n_wts = (long)lmt::pack_bands(b, (size_t)head_floats, fb, nbin, n_mels, gran);
    if ((long)b.size() <= blob_cap) std::memcpy(blob, b.data(), b.size() * sizeof(float));
    return (long)b.size();
}
