// oem_filter_projected.h -- AlignmentFilters::filter_projected for one read's records, as pure host / device functions.
//
// Reference (COMBINE-lab/oarfish, src/util/oarfish_types.rs:1179-1297, records :1142-1164, caller add_projected_group
// :695-715, ProjProbSource src/prog_opts.rs:48-57): the per-record predicate with its discard reason (:1193-1223), the
// tracking of the best similarity and, independently, of the best score (:1225-1237), the verdict (:1240-1248), the
// similarity test (:1256-1260), the clamp of the emitted interval (:1265-1267) and the f32 argument f of
// as_prob = f.exp() (:1274-1282).  The host builder (oem_builder_projected.cpp), the kernels of
// oem_filter_projected_device.hip and the stand-alone program of tests/test_filter_projected.py all call the functions
// below, so they cannot disagree.
//
// The shape is oem_filter.h's: proj_group_measure walks the group twice (predicate, tracking, verdict; then the
// similarity test over the records that passed), proj_group_emit repeats the second walk and hands every kept record
// with its clamped interval and its argument f to the caller.  What differs from filter():
//   - there is no unmapped and no supplementary test, and no_mapping / no_valid_aln are never counted: a group without a
//     retained record, or whose best similarity is not above 0, returns without touching a counter (:1240-1242);
//   - the best similarity is an f64 that starts at f64::MIN, keeps the FIRST maximum (`>`, so a NaN never becomes the
//     best) and fixes aln_frac_at_best = (float)query_aligned_len / (float)read_len, 0 for read_len 0 (:1226-1233);
//   - the test of the second walk is (float)(similarity * (1.0 / best_sim)) >= score_threshold: an f64 product, one cast
//     (:1251, :1256); a NaN similarity fails it;
//   - f is computed here, in IEEE f32 in the order the reference writes it, so the files that include this header are
//     compiled without fast-math and with contraction off.  The i32 score difference wraps, as in a release build.
//
// Argument errors: the reference indexes txps[ref_id] (:1214) and TranscriptInfo::len is non-zero by type, so a ref_id
// that is not below n_txps and a transcript of length 0 are states it cannot be in.  Here either, on ANY record of the
// group (discarded ones included, so that the answer does not depend on the filters), sets kFilterFlagBadRef with the
// record's index.  A record with |aln_score| > 2^24 sets kFilterFlagBigScore: with scores within +-2^24 the difference
// cannot wrap and the gap score table of oem_filter.h applies.
#pragma once

#include "oem_filter.h"

namespace oem {

// what becomes of a projected group
enum : uint32_t { kProjNone = 0,     // empty, nothing retained or best similarity <= 0: no counter moves
                  kProjAlnFrac,      // discard_aln_frac
                  kProjValid };      // valid_best_aln; n_kept may still be 0

constexpr double kProjF64Min = -1.7976931348623157e308; // f64::MIN (:1188)

struct ProjGroup {
    double best_sim = kProjF64Min;
    int32_t best_score = kFilterI32Min; // :1189
    uint32_t verdict = kProjNone;
    uint32_t n_kept = 0;
    uint32_t flags = 0;
    uint32_t bad_record = 0;            // kFilterFlagBadRef: the first such record of the group
};

OEM_HD inline bool proj_source_ok(int32_t s) { return s >= OEM_PROJ_SIMILARITY && s <= OEM_PROJ_COMBINED; }

// The retain predicate (:1193-1223).
OEM_HD inline uint32_t proj_record(const oem_filters &F, const oem_proj_record &x, const uint64_t *txp_len, uint32_t n_txps)
{
    if (x.ref_id >= n_txps || txp_len[x.ref_id] == 0) return kFilterBadRef;
    const bool is_rc = (x.flags & OEM_REC_REVERSE) != 0;
    if (F.which_strand == 2 && !is_rc) return kFilterOri;                                      // :1199
    if (F.which_strand == 1 && is_rc) return kFilterOri;
    if (x.aligned_len < F.min_aligned_len) return kFilterAlnLen;                               // :1206-1209
    if ((int64_t)x.end <= (int64_t)txp_len[x.ref_id] - F.three_prime_clip) return kFilter3p;   // :1214-1217
    if (x.start >= F.five_prime_clip) return kFilter5p;                                        // :1220-1223
    return kFilterPass;
}

// the similarity test of the second walk (:1256): f64 product, one cast
OEM_HD inline bool proj_sim_ok(const oem_filters &F, const oem_proj_record &x, double inv_msim)
{
    return (float)(x.similarity * inv_msim) >= F.score_threshold;
}

// r.aln_score - best_score as a release build takes it (wrapping)
OEM_HD inline int32_t proj_score_diff(int32_t score, int32_t best) { return (int32_t)((uint32_t)score - (uint32_t)best); }

// the integer gap best_score - aln_score of a kept record (never negative while |scores| <= 2^24: best is the maximum)
OEM_HD inline uint64_t proj_gap(int32_t best, const oem_proj_record &x) { return (uint64_t)((int64_t)best - (int64_t)x.aln_score); }

// The log-weight f of a kept record relative to the read's best hit (:1274-1281).
OEM_HD inline float proj_arg(const oem_filters &F, const oem_proj_opts &P, const oem_proj_record &x, double best_sim,
                             int32_t best_score)
{
    if (P.prob_source == OEM_PROJ_SIMILARITY) return (float)(x.similarity - best_sim) * P.beta;         // :1275
    const float by_score = (float)proj_score_diff(x.aln_score, best_score) / F.score_prob_denom;        // :1276
    if (P.prob_source == OEM_PROJ_SCORE) return by_score;
    return by_score + P.beta * (float)(x.similarity - best_sim);                                        // :1278-1279
}

// u32::clamp (:1266-1267); lo <= hi holds for both uses once the transcript's length is not 0
OEM_HD inline uint32_t proj_clamp(uint32_t v, uint32_t lo, uint32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// First walk, verdict, second walk.  An empty group touches nothing (:703-705).
OEM_HD inline ProjGroup proj_group_measure(const oem_filters &F, const oem_proj_record *ag, uint32_t n, uint64_t read_len,
                                           const uint64_t *txp_len, uint32_t n_txps, FilterCounts &c)
{
    ProjGroup g;
    if (n == 0) return g;
    float aln_frac_at_best = 0.f;                                       // :1190
    uint32_t n_pass = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const oem_proj_record &x = ag[i];
        const int64_t s = (int64_t)x.aln_score;
        if (s > kFilterScoreExact || s < -kFilterScoreExact) g.flags |= kFilterFlagBigScore;
        const uint32_t why = proj_record(F, x, txp_len, n_txps);
        if (why == kFilterBadRef) {
            if (!(g.flags & kFilterFlagBadRef)) g.bad_record = i;
            g.flags |= kFilterFlagBadRef;
            continue;
        }
        if (why == kFilterOri) { c.discard_ori += 1; continue; }
        if (why == kFilterAlnLen) { c.discard_aln_len += 1; continue; }
        if (why == kFilter3p) { c.discard_3p += 1; continue; }
        if (why == kFilter5p) { c.discard_5p += 1; continue; }
        if (x.similarity > g.best_sim) {                                // :1226-1233
            g.best_sim = x.similarity;
            aln_frac_at_best = read_len > 0 ? (float)x.query_aligned_len / (float)read_len : 0.f;
        }
        if (x.aln_score > g.best_score) g.best_score = x.aln_score;     // :1234-1236
        ++n_pass;
    }
    if (n_pass == 0 || g.best_sim <= 0.0) return g;                     // :1240-1242
    if (aln_frac_at_best < F.min_aligned_fraction) {                    // :1243-1246
        c.discard_aln_frac += 1;
        g.verdict = kProjAlnFrac;
        return g;
    }
    c.valid_best_aln += 1;                                              // :1248
    g.verdict = kProjValid;
    const double inv_msim = 1.0 / g.best_sim;                           // :1251
    for (uint32_t i = 0; i < n; ++i) {                                  // :1255-1260
        const oem_proj_record &x = ag[i];
        if (proj_record(F, x, txp_len, n_txps) != kFilterPass) continue;
        if (proj_sim_ok(F, x, inv_msim)) g.n_kept += 1;
        else c.discard_score += 1;
    }
    return g;
}

// The second walk again, for a group whose verdict is kProjValid: emit(k, i, x, start, end, f) for the k-th kept record,
// record i of the group, with its clamped interval.
template <typename Emit>
OEM_HD inline void proj_group_emit(const oem_filters &F, const oem_proj_opts &P, const oem_proj_record *ag, uint32_t n,
                                   const uint64_t *txp_len, uint32_t n_txps, double best_sim, int32_t best_score, Emit &&emit)
{
    const double inv_msim = 1.0 / best_sim;
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const oem_proj_record &x = ag[i];
        if (proj_record(F, x, txp_len, n_txps) != kFilterPass) continue;
        if (!proj_sim_ok(F, x, inv_msim)) continue;
        const uint32_t tlen = (uint32_t)txp_len[x.ref_id];              // `as u32` (:1265)
        const uint32_t start = proj_clamp(x.start, 1u, tlen);           // :1266
        const uint32_t end = proj_clamp(x.end, start, tlen);            // :1267
        emit(k++, i, x, start, end, proj_arg(F, P, x, best_sim, best_score));
    }
}

} // namespace oem
