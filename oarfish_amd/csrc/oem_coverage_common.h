// oem_coverage_common.h -- the per-alignment, per-bin and per-read arithmetic of the coverage model, shared by the
// whole-store kernels (oem_coverage_device.hip) and the per-cell ones (oem_coverage_cells.hip).  Same f64 arithmetic
// as the host restatement in oem_builder.cpp:
//   cov_add_interval    TranscriptInfo::add_interval (src/util/oarfish_types.rs:496-538)
//   cov_bin_probs       min coverage + get_normalized_counts_and_lengths (:471-493), then logistic_prob
//                       (src/util/logistic_probability.rs:7-79) or binomial_continuous_prob (binomial_probability.rs:7-224)
//   cov_normalize_read  normalize_read_probs (src/util/normalize_probability.rs:5-74) for one read
// Errors are reported as bits of *err (atomicOr): where the reference panics, the callers return OEM_ERR_STATE.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oem {

enum : uint32_t { kCovErrInterval = 1, kCovErrOlfrac = 2, kCovErrNoBins = 4, kCovErrDegenerate = 8, kCovErrNonFinite = 16 };

// n_bins of a transcript (with_len_and_bin_width, oarfish_types.rs:460-468)
__host__ __device__ inline uint32_t cov_n_bins(uint64_t txp_len, uint32_t bin_width)
{
    return (uint32_t)ceil((double)txp_len / (double)bin_width);
}

// Adds the overlap fraction of every coverage bin the alignment spans into tb (f64 atomics).  Returns false (and adds
// nothing) when the interval lies outside the transcript; the caller then does not count the alignment's weight.
__device__ inline bool cov_add_interval(uint32_t start, uint32_t stop, uint32_t num_intervals, double tlen_f,
                                        double *tb, uint32_t *err)
{
    const double nf = (double)num_intervals;
    const double bw = round(tlen_f / nf);                                          // :501
    start = min(start, stop);                                                      // :502
    stop = max(start, stop);                                                       // :503
    const uint64_t start_bin = (uint64_t)floor(((double)start / tlen_f) * nf);     // :504
    const uint64_t end_bin = (uint64_t)floor(((double)stop / tlen_f) * nf);        // :505
    if (start_bin > end_bin || end_bin > num_intervals) { atomicOr(err, kCovErrInterval); return false; }
    for (uint64_t bi = start_bin; bi < end_bin; ++bi) {                            // :515-536
        const double bidxf = (double)bi;
        const uint32_t cbs = (uint32_t)(bidxf * bw);
        const uint32_t cbe = (uint32_t)fmin((bidxf + 1.0) * bw, tlen_f);
        const uint32_t olap = start <= cbe ? min(stop, cbe) - max(start, cbs) : 0u; // :507-513 (u32)
        const double olfrac = (double)olap / (double)(uint32_t)(cbe - cbs);
        if (olfrac > 1.0 + 2.220446049250313e-16) atomicOr(err, kCovErrOlfrac);    // :524-535: the reference panics
        unsafeAtomicAdd(&tb[bi], olfrac);
    }
    return true;
}

__device__ inline double binomial_bins(const double *tb, uint32_t n, float bwf, float lenf32, double *prob, uint32_t *err)
{
    // binomial_continuous_prob + binomial_probability (binomial_probability.rs:7-224); tb already holds
    // bins + min_cov.  Two sweeps over the bins recompute the f32 counts rather than store them.
    // ln_gamma is the device library's lgamma, not the Lanczos sum of statrs that oem_builder.cpp restates: the
    // device's log is not the host's, so either way the result is an ulp of ln_gamma(709 n) from the reference's.
    const double kZero = 1e-20, kMaxScale = 709.0;
    float count_sum = 0.0f, max_val = 0.0f;
    double distinct_rate = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        const float c = (float)tb[i];
        const float len = fminf(((float)i + 1.0f) * bwf, lenf32) - (float)i * bwf;
        count_sum += c;                                                            // :14
        max_val = i == 0 ? c : fmaxf(max_val, c);                                  // :50
        distinct_rate += (double)c / (double)len;                                  // :184-188
    }
    if (count_sum == 0.0f || distinct_rate == 0.0) {                               // :19-25
        for (uint32_t i = 0; i < n; ++i) prob[i] = 0.0;
        return 0.0;
    }
    float sum_vec = 0.0f;
    for (uint32_t i = 0; i < n; ++i) {                                             // :61-72
        const float c = (float)tb[i];
        sum_vec += c == max_val ? (float)kMaxScale : (float)(((double)c * kMaxScale) / (double)max_val);
    }
    const double ln1 = lgamma((double)sum_vec + 1.0);                              // :75
    double total = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        const float c = (float)tb[i];
        const float len = fminf(((float)i + 1.0f) * bwf, lenf32) - (float)i * bwf;
        const float m = c == max_val ? (float)kMaxScale : (float)(((double)c * kMaxScale) / (double)max_val);
        const double p = (c == 0.0f || len == 0.0f) ? 0.0 : (double)c / ((double)len * distinct_rate); // :27-43
        const double denom = lgamma((double)m + 1.0) + lgamma((double)(sum_vec - m) + 1.0);              // :76-79
        const double num2 = (p > kZero ? log(p) : log(kZero)) * (double)m;                               // :82
        const double q = 1.0 - p;
        const double num3 = (q > kZero ? log(q) : log(kZero)) * (double)(sum_vec - m);                   // :89
        const double res = exp(ln1 - denom + num2 + num3);                                               // :101
        if (isnan(num2) || isinf(num2) || isnan(num3) || isinf(num3) || isnan(res) || isinf(res))
            atomicOr(err, kCovErrNonFinite);                                       // the reference panics (:83-112)
        prob[i] = res;
        total += res;                                                              // :120
    }
    for (uint32_t i = 0; i < n; ++i) {
        prob[i] /= total;                                                          // :124
        if (isnan(prob[i])) atomicOr(err, kCovErrNonFinite);
    }
    return total;
}

// The bin probabilities of one transcript's n bins: tb (the binned coverage) gets the minimum coverage added, tp
// receives the probabilities.  total_weight: alignments binned into tb.
__device__ inline void cov_bin_probs(double *tb, double *tp, uint32_t n, double lenf, uint32_t total_weight, int model,
                                     double growth_rate, uint32_t *err)
{
    if (n == 0) { atomicOr(err, kCovErrNoBins); return; }                          // assert (logistic_probability.rs:54)
    const double min_cov = (double)total_weight / 100.;                            // :55 / binomial :180
    for (uint32_t i = 0; i < n; ++i) tb[i] += min_cov;                             // :56
    // get_normalized_counts_and_lengths (oarfish_types.rs:471-493): f32 counts and bin widths
    const float bwf = (float)round(lenf / (double)n), lenf32 = (float)lenf;
    for (uint32_t i = 0; i < n; ++i) {
        const float bs = (float)i * bwf, be = fminf(((float)i + 1.0f) * bwf, lenf32);
        if (!(be > bs)) { atomicOr(err, kCovErrDegenerate); return; }              // assert (:490)
    }
    if (model == 1) {
        binomial_bins(tb, n, bwf, lenf32, tp, err);
        return;
    }
    double count_sum = 0.0;                                                        // logstic_function (:13-39)
    for (uint32_t i = 0; i < n; ++i) count_sum += (double)(float)tb[i];
    if (count_sum <= 1e-8) {                                                       // :21-23
        for (uint32_t i = 0; i < n; ++i) tp[i] = 0.0;
        return;
    }
    const double expected = count_sum / (double)n;                                 // :27
    for (uint32_t i = 0; i < n; ++i) {
        const double diff = (expected - (double)(float)tb[i]) / expected;          // :32
        double r = 1.0 / (1.0 + exp(-growth_rate * diff));                         // logistic (:7-10)
        r = r < 1e-8 ? 1e-8 : (r > 0.99999 ? 0.99999 : r);
        tp[i] = r;
    }
}

// The bins an alignment reads its probability from: lk(j) gives the alignment's transcript as
// {its bin probabilities, its number of bins, its length}.
struct CovTxpBins {
    const double *tp;
    uint32_t n_bins;
    double tlen;
};

// Alignments [b, e) of one read: per-alignment coverage probability, normalised over the read.
template <typename Lookup>
__device__ inline void cov_normalize_read(uint64_t b, uint64_t e, const uint32_t *__restrict__ aln_start,
                                          const uint32_t *__restrict__ aln_end, double bin_length, Lookup lk,
                                          double *__restrict__ out, uint32_t *err)
{
    double nprob_sum = 0.0;                                                        // normalize_probability.rs:5-74
    for (uint64_t j = b; j < e; ++j) {
        const CovTxpBins x = lk(j);
        if (x.n_bins == 0) { out[j] = 0.0; continue; } // no bins to read (flagged kCovErrNoBins by the bin pass)
        const double *tp = x.tp;
        const double start_aln = (double)aln_start[j], end_aln = (double)aln_end[j], tlen = x.tlen;
        const uint64_t start_bin = (uint64_t)(start_aln / bin_length);             // :25
        uint64_t end_bin = (uint64_t)(end_aln / bin_length);                       // :26-27
        if (end_bin > (uint64_t)x.n_bins - 1) end_bin = (uint64_t)x.n_bins - 1;
        double total_weight = 0.0, cov_prob = 0.0;
        if (start_bin == end_bin) {                                                // :33-35
            const double w = (end_aln - start_aln) / bin_length;
            total_weight = w;
            cov_prob = w * tp[start_bin];
        } else {
            for (uint64_t i = start_bin; i < end_bin; ++i) {                       // :37-46
                const double w = i == start_bin ? (fmin(bin_length * (double)i + bin_length, tlen) - start_aln) / bin_length : 1.0;
                total_weight += w;
                cov_prob += w * tp[i];
            }
        }
        const double expected = cov_prob / total_weight;                           // :58
        if (isnan(cov_prob) || isinf(cov_prob)) atomicOr(err, kCovErrNonFinite); // :49-57 (a 0/0 expected value is not an error there)
        out[j] = expected;
        nprob_sum += expected;
    }
    const double denom = nprob_sum > 0.0 ? nprob_sum : 1.0;                        // :62
    for (uint64_t j = b; j < e; ++j) out[j] /= denom;                              // :65-69
}

} // namespace oem
