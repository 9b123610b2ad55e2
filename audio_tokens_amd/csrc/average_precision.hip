// average_precision.hip -- exact per-class average precision and its mean (mAP), sklearn's recipe in fp64.
//
// Reference call site: utils/metrics_calculator.py:8-33 (MetricsCalculator.compute_metrics / calculate_mAP, called from
// processors/model_trainer.py:96 for the training and the validation set of every epoch): a loop over the classes calling
// sklearn.metrics.average_precision_score(labels[:, i], predictions[:, i]), mean over the classes with a positive.
// For one column sklearn (_binary_clf_curve + precision_recall_curve) sorts by score descending, groups equal scores
// (np.diff != 0, so -0.0 and +0.0 are one group) and sums, over the groups g in that order,
//   AP = sum_g (tp_g - tp_{g-1}) / P * tp_g / cnt_g        tp_g, cnt_g: positives / samples seen up to the end of g
// Here every term is fl(fl(d_g / P) * fl(tp_g / cnt_g)) with integer d_g, tp_g, cnt_g, P (three roundings), and the terms
// of a class are added in fp64 in one fixed order; groups without a positive add nothing.
//
// The kernels and the chunking are ap_stages.h's (shared with at_ranking_metrics_f32, which returns the same bits).
#include "ap_stages.h"

extern "C" int at_average_precision_f32(at_ctx* ctx, const float* scores, int64_t ld_scores, const float* labels,
                                        int64_t ld_labels, int64_t n, int c, double* ap, int64_t* n_pos, double* map,
                                        int32_t* flags, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ap_plan plan;
    int rc = ap_begin(ctx, "at_average_precision_f32", ld_scores, ld_labels, n, c, stream, &plan);
    if (rc) return rc;
    AT_REQUIRE(scores && labels && ap && n_pos && map && flags, "at_average_precision_f32: null pointer");
    AT_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), stream));
    for (int c0 = 0; c0 < c; c0 += plan.cc) {
        const int cn = c - c0 < plan.cc ? c - c0 : plan.cc;
        const uint64_t* sorted;
        if ((rc = ap_sorted_chunk(ctx, plan, scores, ld_scores, labels, ld_labels, n, c0, cn, flags, stream, &sorted))) return rc;
        if ((rc = ap_chunk_terms(plan, sorted, n, cn, ap + c0, n_pos + c0, stream))) return rc;
    }
    AT_LAUNCH(ap_mean_kernel, dim3(1), dim3(64), 0, stream, ap_mean_job{ap, -1, map}, ap_mean_job{nullptr, -1, nullptr},
              n_pos, c);
    return ap_end(ctx, stream);
}
