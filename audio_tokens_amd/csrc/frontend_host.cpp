// frontend_host.cpp -- at_frontend_plan_host: the layout of a batch of clips of unequal length, channel count and
// sample rate for the ragged front end (at_mix_resample_ragged_f32, at_logmel_ragged_f32).  No GPU work.
//
// SpectrogramGenerator.populate_specs (processors/spectrogram_generator.py:86-146 of danavery/audio-tokens) handles
// one clip at a time; this is the table that lets the device handle a batch: where every clip's mono row goes, how
// many frames it has, where they go, and which launch resamples it.
#include <map>
#include <utility>

#include "at_internal.h"

extern "C" int at_frontend_plan_host(const at_frontend_clip_in* clips, int64_t n_clips, int common_sr, int n_fft, int hop,
                                     at_frontend_clip* plan, int32_t* order, at_frontend_group* groups,
                                     int64_t groups_capacity, at_frontend_totals* totals) {
    AT_REQUIRE(totals, "at_frontend_plan_host: totals is null");
    *totals = at_frontend_totals{};
    AT_REQUIRE(n_clips >= 0 && n_clips < (1LL << 31), "at_frontend_plan_host: n_clips out of range");
    AT_REQUIRE(common_sr > 0 && n_fft >= 2 && hop >= 1, "at_frontend_plan_host: bad common_sr / n_fft / hop");
    AT_REQUIRE(groups_capacity >= 0, "at_frontend_plan_host: bad groups_capacity");
    if (n_clips == 0) return AT_OK;
    AT_REQUIRE(clips && plan && order && groups, "at_frontend_plan_host: null pointer");

    std::map<std::pair<int, int>, int> group_of;   // reduced (orig, new) -> group
    int64_t mono = 0, frames = 0, b16 = 0, b32 = 0;
    for (int64_t i = 0; i < n_clips; i++) {
        const at_frontend_clip_in& c = clips[i];
        AT_REQUIRE(c.channels == 1 || c.channels == 2,
                   "at_frontend_plan_host: clip %lld has %d channels (1 or 2; mix more on the caller's side)", (long long)i,
                   c.channels);
        AT_REQUIRE(c.rate > 0 && c.length >= 0 && c.offset >= 0, "at_frontend_plan_host: clip %lld: bad rate, length or offset",
                   (long long)i);
        AT_REQUIRE(c.channels == 1 || c.row_stride >= c.length, "at_frontend_plan_host: clip %lld: row_stride < length",
                   (long long)i);
        int a = c.rate, b = common_sr;
        while (b) { const int t = a % b; a = b; b = t; }
        const int orig = c.rate / a, nw = common_sr / a;
        auto it = group_of.find({orig, nw});
        if (it == group_of.end()) {
            const int g = (int)group_of.size();
            AT_REQUIRE(g < groups_capacity, "at_frontend_plan_host: more than %lld rate pairs", (long long)groups_capacity);
            it = group_of.emplace(std::make_pair(orig, nw), g).first;
            at_frontend_group& G = groups[g];
            G = at_frontend_group{};
            G.orig_freq = c.rate; G.new_freq = common_sr; G.orig = orig; G.nw = nw;
            if (orig == nw) {
                G.mode = AT_FRONTEND_COPY;
                G.out_per_block = AT_RS_COPY_PER_BLOCK;
            } else {
                int o2 = 0, n2 = 0, width = 0;
                int rc = at_resample_taps_host(c.rate, common_sr, &o2, &n2, &width, nullptr, 0);
                if (rc) return rc;
                G.width = width; G.K = 2 * width + orig;
                const long fit = ((long)AT_RS_SEG_FLOATS - G.K) / orig + 1;   // i-steps whose input span fits the segment
                if (fit >= AT_RS_RI) {
                    G.mode = AT_FRONTEND_TILED;
                    G.TI = (int)(fit - fit % AT_RS_RI);
                    G.out_per_block = (int64_t)G.TI * nw;
                } else {
                    G.mode = AT_FRONTEND_SIMPLE;
                    G.out_per_block = 256;
                }
            }
        }
        at_frontend_group& G = groups[it->second];
        at_frontend_clip& r = plan[i];
        r = at_frontend_clip{};
        r.in_offset = c.offset; r.in_row_stride = c.row_stride; r.in_length = c.length;
        r.channels = c.channels; r.group = it->second;
        r.out_length = at_resample_length(c.length, c.rate, common_sr);
        r.mono_offset = mono;
        mono += (r.out_length + 3) & ~(int64_t)3;
        r.too_short = r.out_length <= n_fft / 2;
        const int64_t T = r.too_short ? 0 : at_num_frames(r.out_length, hop);
        AT_REQUIRE(T < (1LL << 31), "at_frontend_plan_host: clip %lld has too many frames", (long long)i);
        r.n_frames = (int32_t)T;
        r.first_frame = frames; r.first_block16 = b16; r.first_block32 = b32;
        frames += T; b16 += (T + 15) / 16; b32 += (T + 31) / 32;
        totals->n_short += r.too_short;
        // resampler blocks: whole tiles of TI input steps (TI * nw output samples), as at_resample_f32 cuts a clip
        r.rs_first_block = G.n_blocks;
        G.n_blocks += (r.out_length + G.out_per_block - 1) / G.out_per_block;
        G.count++;
    }
    const int n_groups = (int)group_of.size();
    int64_t first = 0;
    for (int g = 0; g < n_groups; g++) {
        groups[g].first = first;
        first += groups[g].count;
        groups[g].count = 0;   // refilled below as the cursor
    }
    for (int64_t i = 0; i < n_clips; i++) {
        at_frontend_group& G = groups[plan[i].group];
        order[G.first + G.count++] = (int32_t)i;
    }
    totals->mono_floats = mono; totals->n_frames = frames; totals->n_blocks16 = b16; totals->n_blocks32 = b32;
    totals->n_groups = n_groups;
    return AT_OK;
}
