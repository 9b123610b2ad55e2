// rq_beam.hip -- beam-search residual quantiser on gfx950: at_rq_beam_step_f32 (one stage) and at_rq_beam_encode_f32
// (ResidualQuantizer(max_beam_size = B).compute_codes).  Contract: include/audio_tokens_amd.h, DESIGN.md section 6m.
//
// A row carries b_in partial codes (beams), each with its own residual.  One stage lists, for every beam, the
// k = min(b_out, ksub) nearest words of the stage's codebook -- ONE at_knn_f32 call over the n * b_in residuals, the
// public entry, so every distance is a value that call produces (its fused MFMA sweep for k <= 32 on aligned rows with
// d % 4 == 0 and n * b_in >= 20, its general path otherwise) -- and then keeps the b_out smallest of the b_in * k
// candidates by (distance, parent slot, word), lexicographic and ascending: the select kernel below.
//
// Select kernel: a half-wave (32 lanes) owns a row.  The row's b_in lists of k distances (at_knn_f32 pads a list with
// +inf behind its last listed word, so the distance alone says where a list ends) are staged in LDS, list s at stride
// k | 1 (odd: the 32 heads lie on 32 banks).  Lane s holds the head of list s; b_out rounds of a 32-lane minimum on
// (distance, s) -- float comparison, so -0 and +0 tie and the lower slot wins; a list is already in (distance, word)
// order, so the word needs no comparison -- each followed by one LDS read of the winner's next entry.  Lane t keeps
// the outcome of round t: parent slot, position in the parent's list, distance.  A round that finds only +inf heads
// leaves slot t unfilled (parent 0, word 0, +inf, the flag); every later round does the same.  Then lane t reads the
// word index of its winner from the id list, and all 32 lanes write the new residuals
// r_out[t] = r_in[parent_t] - codebook[word_t], 16 bytes per lane where d % 4 == 0 and the three pointers are 16-byte
// aligned (VEC), one float per lane otherwise; the (parent, word) of the slot a lane works on come by a cross-lane read.
// No atomics; the flag is a plain store of 1.
//
// Encode: blocks of rows sized by a fixed workspace budget (BUDGET_BYTES: two residual buffers of [rows][B][d], the
// lists of one stage, the (parent, word, distance) records of all M stages); per block M stages ping-pong between the
// two residual buffers (stage 0 reads x itself), the last stage writes only slot 0's residual, straight into the
// caller's array; a back-trace kernel follows slot 0 through the parents and writes codes and distances.  The launch
// count per stage does not depend on n; nothing is read back and nothing waits on the host.
#include "at_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WG = 256;              // 8 half-waves: 8 rows per workgroup
constexpr int ROWS_WG = WG / 32;
constexpr int MAX_BEAM = 32;         // the fused top-k of at_knn_f32 stops at k = 32
constexpr size_t BUDGET_BYTES = (size_t)256 << 20;   // workspace of one block of rows of the encode
constexpr int64_t MIN_CALL_ROWS = 20;                // below it at_knn_f32 takes the direct form: no block of a larger call may

__host__ __device__ inline int beam_width(int beam, int ksub, int stages) {   // B_stages = min(beam, ksub^stages)
    int w = 1;
    for (int j = 0; j < stages && w < beam; j++) w *= ksub;
    return w < beam ? w : beam;
}

template <bool VEC>
__global__ void __launch_bounds__(WG)
rq_beam_select_kernel(const float* __restrict__ r_in, long n, int b_in, int d, const float* __restrict__ cb, int k,
                      const long* __restrict__ ids, const float* __restrict__ dis, int b_out, int rslots,
                      float* __restrict__ r_out, int* __restrict__ parent, uint8_t* __restrict__ code,
                      float* __restrict__ dist, int* __restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) float smem[];   // ROWS_WG * b_in * (k | 1) floats
    const int lane = threadIdx.x & 31, sub = threadIdx.x >> 5;
    const long row = (long)blockIdx.x * ROWS_WG + sub;
    const bool live = row < n;
    const long rr = live ? row : n - 1;       // (a half-wave behind the last row recomputes it and stores nothing)
    const int ks = k | 1;
    const float inf = __builtin_inff();

    float* lst = smem + (size_t)sub * b_in * ks;
    const float* drow = dis + rr * (long)b_in * k;
    for (int e = lane; e < b_in * k; e += 32) lst[(e / k) * ks + e % k] = drow[e];
    __syncthreads();

    int pos = 0;
    float head = lane < b_in ? lst[lane * ks] : inf;
    int my_parent = 0, my_pos = -1;
    float my_d = inf;
    for (int t = 0; t < b_out; t++) {
        float bv = head;
        int bs = lane;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const float ov = __shfl_xor(bv, o);
            const int os = __shfl_xor(bs, o);
            if (ov < bv || (ov == bv && os < bs)) {
                bv = ov;
                bs = os;
            }
        }
        const bool filled = bv < inf;
        const int wpos = __shfl(pos, bs, 32);
        if (lane == t) {
            my_d = bv;
            my_parent = filled ? bs : 0;
            my_pos = filled ? wpos : -1;
        }
        if (filled && lane == bs) {
            pos++;
            head = pos < k ? lst[lane * ks + pos] : inf;
        }
    }

    int my_code = 0;
    if (lane < b_out) {
        if (my_pos >= 0) my_code = (int)ids[(rr * (long)b_in + my_parent) * k + my_pos];
        if (live) {
            const long o = row * (long)b_out + lane;
            parent[o] = my_parent;
            code[o] = (uint8_t)my_code;
            dist[o] = my_d;
            if (my_pos < 0 && bad) *bad = 1;
        }
    }

    // the new residuals of the first rslots slots: every lane of the half-wave takes part in every cross-lane read
    const float* rin = r_in + rr * (long)b_in * d;
    float* rout = r_out + rr * (long)rslots * d;
    const int per = VEC ? d / 4 : d;
    const int total = rslots * per;
    for (int e0 = 0; e0 < total; e0 += 32) {
        const int e = e0 + lane;
        const bool ok = e < total;
        const int t = ok ? e / per : 0;
        const int g = ok ? e % per : 0;
        const int p = __shfl(my_parent, t, 32);
        const int c = __shfl(my_code, t, 32);
        if (ok && live) {
            if constexpr (VEC) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(rin + (size_t)p * d + 4 * g);
                const f32x4 w = *reinterpret_cast<const f32x4*>(cb + (size_t)c * d + 4 * g);
                *reinterpret_cast<f32x4*>(rout + (size_t)t * d + 4 * g) = a - w;
            } else {
                rout[(size_t)t * d + g] = rin[(size_t)p * d + g] - cb[(size_t)c * d + g];
            }
        }
    }
}

// Follows slot 0 of the last stage back to stage 0.  Stage m's records are [n][B_{m+1}] at rec + m * n * beam, beam the
// width behind the last stage (min(beam, ksub^(m+1)) is the same for it and for the caller's beam at every m < M).
__global__ void __launch_bounds__(WG)
rq_beam_trace_kernel(long n, int M, int ksub, int beam, const int* __restrict__ parent, const uint8_t* __restrict__ code,
                     const float* __restrict__ dist, uint8_t* __restrict__ codes_out, float* __restrict__ dist_out) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    int s = 0;
    for (int m = M - 1; m >= 0; m--) {
        const int w = beam_width(beam, ksub, m + 1);
        const long o = (long)m * n * beam + i * w + s;
        codes_out[i * M + m] = code[o];
        if (dist_out) dist_out[i * M + m] = dist[o];
        s = parent[o];
    }
}

size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// One stage on the caller's arrays: the lists into `lists` (int64 [n * b_in][k], then float [n * b_in][k] behind them,
// 256-byte aligned), then the select kernel.  r_out holds rslots <= b_out slots per row.
int beam_stage(at_ctx* ctx, const float* r_in, int64_t n, int b_in, int d, const float* cb, int ksub, int b_out,
               int rslots, float* r_out, int32_t* parent, uint8_t* code, float* dist, int32_t* bad, unsigned char* lists,
               hipStream_t stream) {
    const int k = b_out < ksub ? b_out : ksub;
    const size_t nl = (size_t)n * b_in * k;
    int64_t* ids = reinterpret_cast<int64_t*>(lists);
    float* dis = reinterpret_cast<float*>(lists + align256(sizeof(int64_t) * nl));
    const int rc = at_knn_f32(ctx, r_in, n * b_in, d, cb, ksub, k, ids, dis, stream);
    if (rc) return rc;
    const size_t lds = sizeof(float) * ROWS_WG * (size_t)b_in * (k | 1);
    const dim3 grid((unsigned)((n + ROWS_WG - 1) / ROWS_WG));
    if (d % 4 == 0 && at_aligned16(r_in) && at_aligned16(cb) && at_aligned16(r_out)) {
        AT_RAISE_LDS(ctx, rq_beam_select_kernel<true>, lds);
        AT_LAUNCH(rq_beam_select_kernel<true>, grid, dim3(WG), lds, stream, r_in, (long)n, b_in, d, cb, k,
                  reinterpret_cast<const long*>(ids), dis, b_out, rslots, r_out, parent, code, dist, bad);
    } else {
        AT_RAISE_LDS(ctx, rq_beam_select_kernel<false>, lds);
        AT_LAUNCH(rq_beam_select_kernel<false>, grid, dim3(WG), lds, stream, r_in, (long)n, b_in, d, cb, k,
                  reinterpret_cast<const long*>(ids), dis, b_out, rslots, r_out, parent, code, dist, bad);
    }
    return AT_OK;
}

size_t lists_bytes(int64_t n, int b_in, int k) {
    const size_t nl = (size_t)n * b_in * k;
    return align256(sizeof(int64_t) * nl) + align256(sizeof(float) * nl);
}

}  // namespace

extern "C" int at_rq_beam_step_f32(at_ctx* ctx, const float* r_in, int64_t n, int b_in, int d, const float* codebook,
                                   int ksub, int b_out, float* r_out, int32_t* parent, uint8_t* code, float* dist,
                                   int32_t* bad, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_rq_beam_step_f32: ctx is null");
    AT_REQUIRE(n >= 0 && d > 0 && ksub >= 1 && ksub <= 256 && b_in >= 1 && b_in <= MAX_BEAM && b_out >= 1 &&
                   b_out <= MAX_BEAM && b_out <= b_in * ksub,
               "at_rq_beam_step_f32: bad sizes n=%lld d=%d ksub=%d b_in=%d b_out=%d", (long long)n, d, ksub, b_in, b_out);
    if (n == 0) return AT_OK;
    AT_REQUIRE(r_in && codebook && r_out && parent && code && dist, "at_rq_beam_step_f32: null pointer");
    AT_REQUIRE(n <= ((int64_t)1 << 38) / ((int64_t)MAX_BEAM * (d > MAX_BEAM ? d : MAX_BEAM)),
               "at_rq_beam_step_f32: n=%lld too large", (long long)n);
    {
        const char *ia = reinterpret_cast<const char*>(r_in), *oa = reinterpret_cast<const char*>(r_out);
        const size_t ib = sizeof(float) * (size_t)n * b_in * d, ob = sizeof(float) * (size_t)n * b_out * d;
        AT_REQUIRE(oa + ob <= ia || ia + ib <= oa, "at_rq_beam_step_f32: r_out overlaps r_in");
    }
    AT_HIP(hipSetDevice(ctx->device));
    if (bad) AT_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), stream));

    int rc = at_guard_enter(&ctx->guard[AT_GUARD_RQ_BEAM], stream);   // calls of one context share WS_RQ_BEAM_LISTS
    if (rc) return rc;
    const int k = b_out < ksub ? b_out : ksub;
    unsigned char* lists = static_cast<unsigned char*>(at_ws(ctx, WS_RQ_BEAM_LISTS, lists_bytes(n, b_in, k), stream));
    if (!lists) return AT_E_NOMEM;
    rc = beam_stage(ctx, r_in, n, b_in, d, codebook, ksub, b_out, b_out, r_out, parent, code, dist, bad, lists, stream);
    if (rc) return rc;
    return at_guard_leave(&ctx->guard[AT_GUARD_RQ_BEAM], stream);
}

extern "C" int at_rq_beam_encode_f32(at_ctx* ctx, const float* x, int64_t n, int d, int M, int ksub,
                                     const float* codebooks, int beam, uint8_t* codes, float* dist, float* residual,
                                     int32_t* bad, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    AT_REQUIRE(ctx, "at_rq_beam_encode_f32: ctx is null");
    AT_REQUIRE(n >= 0 && d > 0 && M > 0 && ksub >= 1 && ksub <= 256 && beam >= 1 && beam <= MAX_BEAM,
               "at_rq_beam_encode_f32: bad sizes n=%lld d=%d M=%d ksub=%d beam=%d", (long long)n, d, M, ksub, beam);
    if (n == 0) return AT_OK;
    AT_REQUIRE(x && codebooks && codes, "at_rq_beam_encode_f32: null pointer");
    AT_REQUIRE(n <= ((int64_t)1 << 38) / (M > d ? M : d), "at_rq_beam_encode_f32: n=%lld too large", (long long)n);
    if (residual) {
        const char *xa = reinterpret_cast<const char*>(x), *ra = reinterpret_cast<const char*>(residual);
        const size_t bytes = sizeof(float) * (size_t)n * d;
        AT_REQUIRE(ra + bytes <= xa || xa + bytes <= ra, "at_rq_beam_encode_f32: residual overlaps x");
    }
    AT_HIP(hipSetDevice(ctx->device));
    if (bad) AT_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), stream));

    // Rows per block from the budget.  The widest stage decides: B = B_M beams in, k = min(B, ksub) words listed each.
    const int B = beam_width(beam, ksub, M);
    const int kmax = B < ksub ? B : ksub;
    const size_t per_row = 2 * sizeof(float) * (size_t)B * d + (sizeof(int64_t) + sizeof(float)) * (size_t)B * kmax +
                           (sizeof(int32_t) + sizeof(uint8_t) + sizeof(float)) * (size_t)M * B;
    int64_t rows = (int64_t)(BUDGET_BYTES / per_row);
    // at_knn_f32 chooses its direct form by the rows of ITS call: a block of a call with n >= 20 rows never has fewer
    if (rows < 2 * MIN_CALL_ROWS) rows = 2 * MIN_CALL_ROWS;
    if (rows > n) rows = n;

    int rc = at_guard_enter(&ctx->guard[AT_GUARD_RQ_BEAM], stream);   // calls of one context share the WS_RQ_BEAM_* slots
    if (rc) return rc;
    const size_t b_res = align256(sizeof(float) * (size_t)rows * B * d);
    const size_t b_par = align256(sizeof(int32_t) * (size_t)M * rows * B), b_dis = align256(sizeof(float) * (size_t)M * rows * B);
    const size_t b_cod = align256((size_t)M * rows * B);
    unsigned char* res = static_cast<unsigned char*>(at_ws(ctx, WS_RQ_BEAM_RES, 2 * b_res, stream));
    unsigned char* lists = static_cast<unsigned char*>(at_ws(ctx, WS_RQ_BEAM_LISTS, lists_bytes(rows, B, kmax), stream));
    unsigned char* path = static_cast<unsigned char*>(at_ws(ctx, WS_RQ_BEAM_PATH, b_par + b_dis + b_cod, stream));
    if (!res || !lists || !path) return AT_E_NOMEM;
    float* rbuf[2] = {reinterpret_cast<float*>(res), reinterpret_cast<float*>(res + b_res)};
    int32_t* parent = reinterpret_cast<int32_t*>(path);
    float* sdist = reinterpret_cast<float*>(path + b_par);
    uint8_t* scode = path + b_par + b_dis;

    for (int64_t r0 = 0; r0 < n;) {
        int64_t m_rows = n - r0 < rows ? n - r0 : rows;
        const int64_t left = n - r0 - m_rows;
        if (left > 0 && left < MIN_CALL_ROWS) m_rows -= MIN_CALL_ROWS;   // (rows >= 40: the block keeps 20 rows or more)
        const float* rin = x + r0 * d;
        int b_in = 1;
        for (int m = 0; m < M; m++) {
            const int b_out = beam_width(beam, ksub, m + 1);
            const bool last = m + 1 == M;
            float* rout = last ? (residual ? residual + r0 * d : nullptr) : rbuf[m & 1];
            const int rslots = last ? (residual ? 1 : 0) : b_out;
            const size_t o = (size_t)m * m_rows * B;
            rc = beam_stage(ctx, rin, m_rows, b_in, d, codebooks + (size_t)m * ksub * d, ksub, b_out, rslots, rout, parent + o,
                            scode + o, sdist + o, bad, lists, stream);
            if (rc) return rc;
            rin = rout;
            b_in = b_out;
        }
        AT_LAUNCH(rq_beam_trace_kernel, dim3((unsigned)((m_rows + WG - 1) / WG)), dim3(WG), 0, stream, (long)m_rows, M, ksub,
                  B, parent, scode, sdist, codes + r0 * M, dist ? dist + r0 * M : nullptr);
        r0 += m_rows;
    }
    return at_guard_leave(&ctx->guard[AT_GUARD_RQ_BEAM], stream);
}
