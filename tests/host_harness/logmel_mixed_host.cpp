// logmel_mixed_host.cpp -- runs the plan and the per-lane passes of audio_tokens_amd/csrc/logmel_mixed_core.h on the
// host, 64 "lanes" one after the other, so tests can check the index algebra of every n_fft without a GPU.
// TEST INFRASTRUCTURE (built on the fly by tests/test_logmel_mixed_host.py with g++).
#include <utility>
#include <vector>

#include "../../audio_tokens_amd/csrc/logmel_mixed_core.h"

using namespace lmx;

namespace {

struct NoBarrier {
    void operator()() const {}
};
const Lanes kAll{0, 64};

// what the kernel does with a frame, with all 64 lanes run one after the other: on return `*z_out` points at Z (M
// complex points) and `*free_out` at the buffer the kernel writes the power bins to
struct Frame {
    Plan pl;
    std::vector<float> tw, chirp, bhat, a, b;
    explicit Frame(const Plan& plan) : pl(plan), tw(2 * (size_t)plan.P), a(2 * (size_t)plan.P), b(2 * (size_t)plan.P) {
        twiddle_table(pl.P, tw.data());
        if (pl.form == FORM_BLUESTEIN) {
            chirp.resize(2 * (size_t)pl.M);
            bhat.resize(2 * (size_t)pl.P);
            bluestein_tables(pl.M, pl.P, chirp.data(), bhat.data());
        }
    }
    void transform(const float* z, float** z_out, float** free_out) {
        float *cur = a.data(), *oth = b.data();
        if (pl.form == FORM_MIXED)
            frame_transform<false>(kAll, pl.M, pl.P, pl.npass, pl.packed, tw.data(), nullptr, nullptr, LdsLoad{z}, cur, oth,
                                   NoBarrier{});
        else
            frame_transform<true>(kAll, pl.M, pl.P, pl.npass, pl.packed, tw.data(), chirp.data(), bhat.data(), LdsLoad{z},
                                  cur, oth, NoBarrier{});
        *z_out = cur;
        *free_out = oth;
    }
};

}  // namespace

// out: form, P, npass, radix[11]
extern "C" void lmx_host_plan(int n_fft, int force_fallback, int* out) {
    const Plan pl = make_plan(n_fft, force_fallback != 0);
    out[0] = pl.form;
    out[1] = pl.P;
    out[2] = pl.npass;
    for (int i = 0; i < MAX_PASSES; i++) out[3 + i] = plan_radix(pl.packed, i);
}

// the M = n_fft/2-point complex transform of z (interleaved re, im)
extern "C" void lmx_host_fft(int n_fft, int force_fallback, const float* z, float* Z) {
    Frame f(make_plan(n_fft, force_fallback != 0));
    float *r, *free_;
    f.transform(z, &r, &free_);
    for (int i = 0; i < n_fft; i++) Z[i] = r[i];
}

// |rfft(frame)|^2, n_fft/2 + 1 bins, of an already windowed frame; the bins are written where the kernel writes them
// (the buffer the transform left free)
extern "C" void lmx_host_power(int n_fft, int force_fallback, const float* frame, float* power) {
    Frame f(make_plan(n_fft, force_fallback != 0));
    const int M = f.pl.M;
    std::vector<float> twn(2 * (size_t)M);
    untangle_table(n_fft, twn.data());
    float *Z, *pw;
    f.transform(frame, &Z, &pw);   // z[m] = (x[2m], x[2m+1]): the frame as it lies in memory
    untangle_lanes(kAll, M, Z, twn.data(), pw, NoBarrier{});
    for (int k = 0; k <= M; k++) power[k] = pw[k];
}

// every (j, NS) the passes can meet: the fp32 remainder equals the integer one; returns the number of mismatches
extern "C" int lmx_host_check_mod(void) {
    int bad = 0;
    for (int NS = 1; NS <= 4096; NS++) {
        const float inv = 1.0f / (float)NS;
        for (int j = 0; j < 4096; j++) bad += mod_ns(j, NS, inv) != j % NS;
    }
    return bad;
}
