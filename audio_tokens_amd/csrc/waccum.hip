// waccum.hip -- compute_centroids (accumulate) with per-row weights on gfx950: at_centroid_accum_weighted_f32.
//
// The contract: for cluster c with members i0 < i1 < ... (ascending row),
//     sums[c][f] = the chain s <- fmaf(x[i][f], w[i], s) from +0, one rounding per member,
//     wsums[c]   = the chain s <- s + w[i] from +0, in the same order.
// The kernels are the WEIGHTED = true forms of accum_kernels.h, the ones accum.hip instantiates with false; this file
// is their host driver.  It is an object of its own because these forms are built without packed-fp32 instructions
// (Makefile, NOPK_OBJS).
//
// Member lists: a stable radix sort of (id, row) pairs (at_sort.h) and the segment starts by binary search, as in the
// sort strategy of accum.hip -- in workspace slots of ITS OWN (WS_WACC_*), so a weighted call never touches what
// at_centroid_accum_f32 or its side stream are using.  Calls of one context share those slots: a call on another
// stream than the previous one waits for it (AT_GUARD_WACC).  Everything is queued on the caller's stream, in
// sequence: sort, offsets (which also list the long clusters), short lists, long lists.  accum.hip's predicted early
// lists, bucket strategy and side stream are left out on purpose.
#include <cstdlib>
#include <cstring>

#include "accum_kernels.h"
#include "at_internal.h"
#include "at_sort.h"

namespace {

using Shape = AccumShape<true>;
constexpr int LONG_GRID = 64;   // workgroups per feature slice; they stride over the long clusters

int waccum_queue(at_ctx* ctx, const float* x, const float* w, long n, int d, const long* ids, int k, float* sums, float* wsums,
                 uint32_t* order_out, uint32_t* sorted_ids_out, hipStream_t stream) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    uint32_t* keys_a = static_cast<uint32_t*>(at_ws(ctx, WS_WACC_KEYS_A, nn * 4, stream));
    uint32_t* keys_b = static_cast<uint32_t*>(at_ws(ctx, WS_WACC_KEYS_B, nn * 4, stream));
    uint32_t* vals_a = static_cast<uint32_t*>(at_ws(ctx, WS_WACC_VALS_A, nn * 4, stream));
    uint32_t* vals_b = static_cast<uint32_t*>(at_ws(ctx, WS_WACC_VALS_B, nn * 4, stream));
    // WS_WACC_SEG, in words: offsets[k + 2] | longs[k + 1]
    uint32_t* offsets = static_cast<uint32_t*>(at_ws(ctx, WS_WACC_SEG, ((size_t)2 * k + 3) * 4, stream));
    if (!keys_a || !keys_b || !vals_a || !vals_b || !offsets) return AT_E_NOMEM;
    int* longs = reinterpret_cast<int*>(offsets + k + 2);

    // The feature-sliced kernel reads 16-byte slices of the rows: without them every list is a short one, walked
    // by the scalar-lane form of the short kernel (same order, same bits).
    const bool al = at_aligned16(x), long_ok = d % 4 == 0 && al;
    const uint32_t long_list = long_ok ? Shape::LONG_LIST : UINT32_MAX;
    const long max_long = long_ok ? n / ((long)Shape::LONG_LIST + 1) : 0;   // as many lists can be that long
    const int vec = d % 4 == 0 && d >= 256 && al ? 4 : d % 2 == 0 && d >= 128 && al ? 2 : 1;
    const int slabs = (d + 64 * vec - 1) / (64 * vec);

    const uint32_t *order = vals_a, *sorted_keys = keys_a;
    if (n > 0) {
        AT_LAUNCH(make_keys_kernel, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, stream, ids, n, k, keys_a, vals_a);
        unsigned bits = 1;
        while ((1u << bits) <= (unsigned)k) bits++;  // keys take values 0..k
        rocprim::double_buffer<uint32_t> kb(keys_a, keys_b);
        rocprim::double_buffer<uint32_t> vb(vals_a, vals_b);
        AT_TRY(at_sort_pairs(ctx, WS_WACC_TMP, kb, vb, (size_t)n, 0, bits, stream));
        order = vb.current(), sorted_keys = kb.current();
    }
    if (max_long > 0) AT_HIP(hipMemsetAsync(longs, 0, 4, stream));
    AT_LAUNCH(segment_offsets_kernel, dim3((k + 1 + WG - 1) / WG), dim3(WG), 0, stream, sorted_keys, n, k, long_list, offsets,
              max_long > 0 ? longs : nullptr);
    auto* short_kernel = vec == 4 ? centroid_accum_kernel<4, true> : vec == 2 ? centroid_accum_kernel<2, true> : centroid_accum_kernel<1, true>;
    AT_LAUNCH(short_kernel, dim3((unsigned)(((long)k * slabs + WG / 64 - 1) / (WG / 64))), dim3(WG), 0, stream, x, w, d, order,
              offsets, k, slabs, long_list, sums, wsums);
    if (max_long > 0)
        // (list mode: `longs` has the layout of accum.hip's late list; no early lists, no marks; at most k slots)
        AT_LAUNCH(centroid_accum_long_kernel<true>, dim3((unsigned)(max_long < LONG_GRID ? max_long : LONG_GRID), d / 4), dim3(WG), 0,
                  stream, x, w, d, order, offsets, long_list, sums, wsums, k, 0, longs, nullptr, nullptr, 0u, 0, k);
    if (n > 0) {
        const size_t bytes = sizeof(uint32_t) * (size_t)n;
        if (order_out) AT_HIP(hipMemcpyAsync(order_out, order, bytes, hipMemcpyDeviceToDevice, stream));
        if (sorted_ids_out) AT_HIP(hipMemcpyAsync(sorted_ids_out, sorted_keys, bytes, hipMemcpyDeviceToDevice, stream));
    }
    return AT_OK;
}

}  // namespace

extern "C" {

int at_centroid_accum_weighted_f32(at_ctx* ctx, const float* x, const float* w, int64_t n, int d, const int64_t* ids, int k,
                                   float* sums, float* wsums, uint32_t* order_out, uint32_t* sorted_ids_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AT_REQUIRE(ctx, "at_centroid_accum_weighted_f32: ctx is null");
    AT_REQUIRE(n >= 0 && n < (int64_t)UINT32_MAX && d > 0 && k > 0 && k < (1 << 30),
               "at_centroid_accum_weighted_f32: bad sizes n=%lld d=%d k=%d", (long long)n, d, k);
    AT_REQUIRE(sums && wsums && (n == 0 || (x && w && ids)), "at_centroid_accum_weighted_f32: null pointer");
    AT_HIP(hipSetDevice(ctx->device));
    AT_TRY(at_guard_enter(&ctx->guard[AT_GUARD_WACC], stream));   // calls of one context share the WS_WACC_* slots
    const int rc = waccum_queue(ctx, x, w, (long)n, d, reinterpret_cast<const long*>(ids), k, sums, wsums, order_out,
                                sorted_ids_out, stream);
    const int grc = at_guard_leave(&ctx->guard[AT_GUARD_WACC], stream);
    return rc != AT_OK ? rc : grc;
}

// include/at_debug.h: the sizes at which the weighted accumulation changes its path (NULL skips a field)
int at_waccum_limits(int* short_batch, int* short_batch_wide, int* long_list, int* ring_chunk) {
    if (short_batch) *short_batch = Shape::RB;
    if (short_batch_wide) *short_batch_wide = Shape::RB_WIDE;
    if (long_list) *long_list = (int)Shape::LONG_LIST;
    if (ring_chunk) *ring_chunk = Shape::CHUNK;
    return AT_OK;
}

}  // extern "C"
