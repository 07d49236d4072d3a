// capi_stats.cpp -- host statistics entry points of the C-ABI (include/cgpt.h).
#include "../../include/cgpt.h"
#include "common_host.h"
#include "stats.h"

extern "C" {

static cgpt_status certify_rows(const char* who, const int64_t* csel, const int64_t* cest, int64_t row_stride, int64_t num_images,
                                int32_t num_classes, int64_t n, double alpha, double scale, int32_t law, int32_t* labels_out,
                                double* radii_out) {
    if (law != CGPT_NOISE_GAUSSIAN && law != CGPT_NOISE_UNIFORM)
        return cgpt_fail(CGPT_ERR_INVALID, std::string(who) + ": law must be CGPT_NOISE_GAUSSIAN or CGPT_NOISE_UNIFORM");
    if (!csel || !cest || !labels_out || !radii_out || num_images < 0 || num_classes < 1 || n < 1 || !(alpha > 0.0 && alpha < 1.0))
        return cgpt_fail(CGPT_ERR_INVALID, std::string(who) + ": bad argument");
    for (int64_t i = 0; i < num_images; ++i) {
        int label; double radius;
        cgpt_stats::certify_from_counts(csel + i * row_stride, cest + i * row_stride, num_classes, n, alpha, scale, &label, &radius, law);
        labels_out[i] = label; radii_out[i] = radius;
    }
    return CGPT_OK;
}

cgpt_status cgpt_certify_from_counts(const int64_t* counts_selection, const int64_t* counts_estimation,
                                     int32_t num_classes, int64_t n, double alpha, double sigma,
                                     int32_t* label_out, double* radius_out) {
    return certify_rows("cgpt_certify_from_counts", counts_selection, counts_estimation, 0, 1, num_classes, n, alpha, sigma,
                        CGPT_NOISE_GAUSSIAN, label_out, radius_out);
}

cgpt_status cgpt_certify_many_from_counts(const int64_t* counts, int64_t num_images, int32_t num_classes, int64_t n, double alpha,
                                          double sigma, int32_t* labels_out, double* radii_out) {
    return certify_rows("cgpt_certify_many_from_counts", counts, counts ? counts + num_classes : nullptr, 2 * (int64_t)num_classes,
                        num_images, num_classes, n, alpha, sigma, CGPT_NOISE_GAUSSIAN, labels_out, radii_out);
}

cgpt_status cgpt_certify_many_from_counts_law(const int64_t* counts, int64_t num_images, int32_t num_classes, int64_t n, double alpha,
                                              double scale, int32_t law, int32_t* labels_out, double* radii_out) {
    return certify_rows("cgpt_certify_many_from_counts_law", counts, counts ? counts + num_classes : nullptr, 2 * (int64_t)num_classes,
                        num_images, num_classes, n, alpha, scale, law, labels_out, radii_out);
}

cgpt_status cgpt_predict_from_counts(const int64_t* counts, int32_t num_classes, double alpha, int32_t* label_out) {
    // the reference indexes top2[1] (smoothing.py:75): it needs at least two classes
    if (!counts || !label_out || num_classes < 2 || !(alpha > 0.0 && alpha < 1.0))
        return cgpt_fail(CGPT_ERR_INVALID, "cgpt_predict_from_counts: bad argument (num_classes >= 2 required)");
    *label_out = cgpt_stats::predict_from_counts(counts, num_classes, alpha);
    return CGPT_OK;
}

double cgpt_lower_confidence_bound(int64_t NA, int64_t N, double alpha) { return cgpt_stats::cp_lower_bound(NA, N, alpha); }
double cgpt_binom_test(int64_t x, int64_t n, double p) { return cgpt_stats::binom_test_two_sided(x, n, p); }
double cgpt_norm_ppf(double p) { return cgpt_stats::norm_ppf(p); }

}  // extern "C"
