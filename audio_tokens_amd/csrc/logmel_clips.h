// logmel_clips.h -- the one place that maps a unit of log-mel work to its clip.
//
// Every kernel of the family walks a flat index space -- output frames (the general kernels, the pieces of the min-max
// passes) or blocks of 16 / 32 frames of one clip (the tuned n_fft = 512 kernel) -- and asks the same question: whose
// is this, and what is that clip's geometry?  Two maps answer it through one interface:
//   UniformClips  n_clips rows of L samples, wave_stride apart, T frames each (at_logmel_f32): by division;
//   PlanClips     the clips of an at_frontend_plan_host plan, each with its own length, frames and place in the
//                 intermediate buffer and in the output (at_logmel_ragged_f32): by binary search over a prefix.
// A kernel is a template on the map type; has_flags says whether the map carries per-clip NaN / Inf flags to set.
// The output of either map is one flat run of frames, clip after clip: the clip whose first output frame is `base`
// owns [base, base + T) x n_mels floats of it in both layouts.
// Host-compilable (tests/host_harness/logmel_clips_host.cpp runs the lookups without a GPU).
#pragma once
#include <cstdint>

#include "../../include/audio_tokens_amd.h"

#if defined(__HIPCC__)
#define AT_LMC_HD __host__ __device__ __forceinline__
#else
#define AT_LMC_HD inline
#endif

namespace lmc {

// One frame (by_frame) or one block of frames (by_block): whose it is, and that clip's geometry.
struct ClipAt {
    long clip;
    int t, T;               // the frame / the block's first frame within the clip, frames of the clip
    const float* w;         // the clip's samples
    long L;
    long base;              // the clip's first output frame
};

// The clip whose prefix is the last one <= x.  `prefix` is one of at_frontend_clip's exclusive prefix sums
// (first_frame, first_block16, first_block32) and 0 <= x < their total.  A clip without frames shares its prefix with
// the clip behind it and is never found: the search keeps the LAST clip whose prefix is <= x, and behind every run of
// empty clips comes one that has frames (x < total), or x would belong to the clip in front of the run.
AT_LMC_HD long find_clip(const at_frontend_clip* plan, long n_clips, int64_t at_frontend_clip::*prefix, long x) {
    long lo = 0, hi = n_clips;
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (plan[mid].*prefix <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct UniformClips {
    static constexpr bool has_flags = false;
    const float* wave;
    long L, wave_stride;
    int T;
    AT_LMC_HD ClipAt at(long clip, int t) const { return {clip, t, T, wave + clip * wave_stride, L, clip * T}; }
    AT_LMC_HD ClipAt by_frame(long g) const {
        const long clip = g / T;
        return at(clip, (int)(g - clip * T));
    }
    // fpb: 16 or 32 frames per block
    AT_LMC_HD ClipAt by_block(long blk, int fpb) const {
        const int per_clip = (T + fpb - 1) >> (fpb == 32 ? 5 : 4);
        const long clip = blk / per_clip;
        return at(clip, (int)(blk - clip * per_clip) * fpb);
    }
};

struct PlanClips {
    static constexpr bool has_flags = true;
    const float* wave;              // the intermediate buffer
    const at_frontend_clip* plan;
    long n_clips;
    int32_t* flags;                 // [n_clips]: set where a value stored for the clip is not finite
    AT_LMC_HD ClipAt at(long clip, long t) const {
        const at_frontend_clip& c = plan[clip];
        return {clip, (int)t, c.n_frames, wave + c.mono_offset, c.out_length, c.first_frame};
    }
    AT_LMC_HD ClipAt by_frame(long g) const {
        const long clip = find_clip(plan, n_clips, &at_frontend_clip::first_frame, g);
        return at(clip, g - plan[clip].first_frame);
    }
    AT_LMC_HD ClipAt by_block(long blk, int fpb) const {
        int64_t at_frontend_clip::*const prefix = fpb == 32 ? &at_frontend_clip::first_block32 : &at_frontend_clip::first_block16;
        const long clip = find_clip(plan, n_clips, prefix, blk);
        return at(clip, (blk - plan[clip].*prefix) * fpb);
    }
};

// Where the clip that owns output frame g ends (one past its last frame), and which clip it is: the piece walk of the
// min-max passes.
template <typename Clips>
AT_LMC_HD long clip_end(const Clips& clips, long g, long* clip) {
    const ClipAt c = clips.by_frame(g);
    *clip = c.clip;
    return c.base + c.T;
}

}  // namespace lmc
