// The clip maps of audio_tokens_amd/csrc/logmel_clips.h run on the host: every lookup the log-mel kernels make,
// for a list of frames or blocks at a time (tests/test_logmel_clips_host.py).
// out: six int64 per query -- clip, frame within the clip, frames of the clip, offset of the clip's samples from
// `wave` in floats, samples of the clip, first output frame of the clip.
#include "../../audio_tokens_amd/csrc/logmel_clips.h"

namespace {

void put(const lmc::ClipAt& c, const float* wave, int64_t* out) {
    out[0] = c.clip; out[1] = c.t; out[2] = c.T; out[3] = c.w - wave; out[4] = c.L; out[5] = c.base;
}

// fpb = 0: x are output frames (by_frame); 16 or 32: x are blocks of that many frames (by_block)
template <typename Clips>
void lookups(const Clips& clips, const float* wave, const int64_t* x, int64_t m, int fpb, int64_t* out) {
    for (int64_t i = 0; i < m; i++) put(fpb ? clips.by_block(x[i], fpb) : clips.by_frame(x[i]), wave, out + 6 * i);
}

// out: two int64 per frame -- where the clip that owns it ends, and which clip that is
template <typename Clips>
void ends(const Clips& clips, const int64_t* g, int64_t m, int64_t* out) {
    for (int64_t i = 0; i < m; i++) {
        long clip = -1;
        out[2 * i] = lmc::clip_end(clips, g[i], &clip);
        out[2 * i + 1] = clip;
    }
}

}  // namespace

extern "C" {

void lmc_host_plan_lookups(const at_frontend_clip* plan, int64_t n_clips, const float* wave, const int64_t* x, int64_t m,
                           int fpb, int64_t* out) {
    lookups(lmc::PlanClips{wave, plan, (long)n_clips, nullptr}, wave, x, m, fpb, out);
}
void lmc_host_plan_ends(const at_frontend_clip* plan, int64_t n_clips, const int64_t* g, int64_t m, int64_t* out) {
    ends(lmc::PlanClips{nullptr, plan, (long)n_clips, nullptr}, g, m, out);
}
void lmc_host_uniform_lookups(const float* wave, int64_t L, int64_t wave_stride, int T, const int64_t* x, int64_t m, int fpb,
                              int64_t* out) {
    lookups(lmc::UniformClips{wave, L, wave_stride, T}, wave, x, m, fpb, out);
}
void lmc_host_uniform_ends(int T, const int64_t* g, int64_t m, int64_t* out) {
    ends(lmc::UniformClips{nullptr, 0, 0, T}, g, m, out);
}
int lmc_host_has_flags(int plan) { return plan ? lmc::PlanClips::has_flags : lmc::UniformClips::has_flags; }

}
