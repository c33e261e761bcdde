// oem_filter.h -- AlignmentFilters::filter for one read's records, as pure host / device functions.
//
// Reference (COMBINE-lab/oarfish v0.10.3, src/util/oarfish_types.rs:955-1130): the per-record predicate with its
// discard reason (:985-1069), the best-score tracking (:1053-1063), the group verdict (:1071-1092), the score test and
// the conditional probability as_prob = expf((score - best) / D) (:1095-1118).  Nothing from HIP is needed: the host
// builder (oem_builder.cpp: oem_builder_add_group, oem_builder_add_groups), the kernels of oem_filter_device.hip and the
// stand-alone program of tests/test_filter_groups.py all call the functions below, so they cannot disagree.
//
// A group is walked twice.  filter_group_measure applies the predicate to every record, counts the discards, tracks the
// best score and reaches the verdict; then it walks the records that passed again, applies the score test and counts what
// stays.  filter_group_emit repeats the second walk and hands every retained record to the caller.  The tracking keeps
// the FIRST maximum (the comparison is `score > best`), and seq_len is the first record's that has one (:979-982).
//
// All f32 arithmetic is plain IEEE, in the order the reference writes it: (float)aln_span / (float)seq_len,
// 1.0f / mscore, fscore * inv_max_score >= thr.  These three comparisons decide which records are kept, so the files
// that include this header are compiled without fast-math, without approximate division and with contraction off.
//
// The probability is never computed on the device.  expf is the host libm's by definition (what Rust's f32::exp lowers
// to), and libm's expf is not the correctly rounded function, so no independent exponential can promise bit equality.
// The scores are integers: for |score| <= 2^24 both (float)score and (float)best are exact and their f32 difference is
// the correctly rounded -(best - score), i.e. (float)(-g) with g the integer gap.  filter_prob_table fills, on the
// host, tab[g] = expf((float)(-g) / D) for g = 0, 1, ... up to and including the first g whose value is +0.0f (about
// 104 D + 1 entries; expf is 0 from there on, the argument only falls); filter_prob looks as_prob up by g and gives
// +0.0f beyond the table's end.  A batch goes through the host loop instead when D is not finite and positive, when
// the table would need more than kFilterTabMax entries, or when a mapped record with a score has
// |(int32_t)score| > 2^24 (the device pass detects that: kFilterFlagBigScore); the result is the same either way.
#pragma once

#include <stdint.h>

#include "../../include/oarfish_em.h"

#ifndef OEM_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define OEM_HD __host__ __device__
#else
#define OEM_HD
#endif
#endif

#include <math.h>

#include <vector>

namespace oem {

// why a record leaves in the first walk (kFilterPass: it does not)
enum : uint32_t { kFilterPass = 0, kFilterUnmapped, kFilterOri, kFilterSupp, kFilterAlnLen, kFilter3p, kFilter5p, kFilterBadRef };
// what becomes of the group
enum : uint32_t { kGroupEmpty = 0, kGroupNoMapping, kGroupNoValidAln, kGroupAlnFrac, kGroupValid };
// what the walk saw besides
enum : uint32_t { kFilterFlagBadRef = 1u,    // a mapped record with ref_id >= n_txps: an argument error
                  kFilterFlagBigScore = 2u }; // a mapped record with a score beyond +-2^24: the gap table does not apply

constexpr int32_t kFilterI32Min = -2147483647 - 1;
constexpr int64_t kFilterScoreExact = 1ll << 24;
constexpr uint64_t kFilterTabMax = 1ull << 22;

// A group's contributions to the discard table, in the order of oem_discard_table's fields.
struct FilterCounts {
    uint32_t discard_5p = 0, discard_3p = 0, discard_score = 0, discard_aln_frac = 0, discard_aln_len = 0, discard_ori = 0,
             discard_supp = 0, valid_best_aln = 0, no_mapping = 0, no_valid_aln = 0;
};
constexpr int kFilterCounters = 10;
static_assert(sizeof(FilterCounts) == kFilterCounters * sizeof(uint32_t), "FilterCounts mirrors oem_discard_table");
static_assert(sizeof(oem_discard_table) == kFilterCounters * sizeof(uint64_t), "oem_discard_table has ten counters");

struct FilterGroup {
    int32_t best = kFilterI32Min; // best retained score (:963)
    uint32_t verdict = kGroupEmpty;
    uint32_t n_kept = 0;          // what add_group returns
    uint32_t flags = 0;
    uint32_t bad_record = 0;      // kFilterFlagBadRef: the first such record of the group
};

OEM_HD inline int32_t filter_score_i32(const oem_aln_record &x, int32_t if_none)
{
    return (x.flags & OEM_REC_HAS_SCORE) ? (int32_t)x.score : if_none;
}

// The retain predicate (:985-1069).  txp_len is read only for a record that reaches the 3' test.
OEM_HD inline uint32_t filter_record(const oem_filters &F, const oem_aln_record &x, const uint64_t *txp_len, uint32_t n_txps)
{
    if (x.flags & OEM_REC_UNMAPPED) return kFilterUnmapped;                                    // :987
    if (x.ref_id >= n_txps) return kFilterBadRef;
    const bool is_rc = (x.flags & OEM_REC_REVERSE) != 0;                                       // :997
    if (F.which_strand == 2 && !is_rc) return kFilterOri;                                      // :1008-1011
    if (F.which_strand == 1 && is_rc) return kFilterOri;                                       // :1013-1016
    if (x.flags & OEM_REC_SUPPLEMENTARY) return kFilterSupp;                                   // :1022-1026
    if (x.aln_span < F.min_aligned_len) return kFilterAlnLen;                                  // :1029-1033
    if ((int64_t)x.aln_end <= (int64_t)txp_len[x.ref_id] - F.three_prime_clip) return kFilter3p; // :1036-1041
    if (x.aln_start >= F.five_prime_clip) return kFilter5p;                                    // :1044-1048
    return kFilterPass;
}

// the score test of the second walk (:1102-1109); a record without a score counts as 0 (unwrap_or(0))
OEM_HD inline bool filter_score_ok(const oem_filters &F, const oem_aln_record &x, float inv_max_score)
{
    const float fscore = (float)filter_score_i32(x, 0);
    return (fscore * inv_max_score) >= F.score_threshold;
}

// the integer gap best - score of a record that passed both walks (never negative: best is the maximum)
OEM_HD inline uint64_t filter_gap(int32_t best, const oem_aln_record &x)
{
    return (uint64_t)((int64_t)best - (int64_t)filter_score_i32(x, 0));
}

OEM_HD inline float filter_prob(const float *tab, uint64_t n_tab, uint64_t gap) { return gap < n_tab ? tab[gap] : 0.0f; }

// First walk, verdict, second walk.  An empty group touches nothing (add_group: `if !ag.is_empty()`, :677).
OEM_HD inline FilterGroup filter_group_measure(const oem_filters &F, const oem_aln_record *ag, uint32_t n,
                                                const uint64_t *txp_len, uint32_t n_txps, FilterCounts &c)
{
    FilterGroup g;
    if (n == 0) return g;
    float aln_frac_at_best = 0.f;                                       // :966
    uint32_t aln_len_at_best = 0, n_mapped_in = 0, n_pass = 0;          // :969, :974
    uint32_t seq_len = 0;                                               // :979-982
    for (uint32_t i = 0; i < n; ++i)
        if (ag[i].seq_len >= 0) { seq_len = (uint32_t)ag[i].seq_len; break; }
    for (uint32_t i = 0; i < n; ++i) {
        const oem_aln_record &x = ag[i];
        const uint32_t why = filter_record(F, x, txp_len, n_txps);
        if (why == kFilterUnmapped) continue;
        ++n_mapped_in;
        if (x.flags & OEM_REC_HAS_SCORE) {
            const int64_t s = (int64_t)(int32_t)x.score;
            if (s > kFilterScoreExact || s < -kFilterScoreExact) g.flags |= kFilterFlagBigScore;
        }
        if (why == kFilterBadRef) {
            if (!(g.flags & kFilterFlagBadRef)) g.bad_record = i;
            g.flags |= kFilterFlagBadRef;
            continue;
        }
        if (why == kFilterOri) { c.discard_ori += 1; continue; }
        if (why == kFilterSupp) { c.discard_supp += 1; continue; }
        if (why == kFilterAlnLen) { c.discard_aln_len += 1; continue; }
        if (why == kFilter3p) { c.discard_3p += 1; continue; }
        if (why == kFilter5p) { c.discard_5p += 1; continue; }
        const int32_t score = filter_score_i32(x, kFilterI32Min);       // :994
        if (score > g.best) {                                           // :1053-1063
            g.best = score;
            aln_len_at_best = x.aln_span;
            aln_frac_at_best = seq_len > 0 ? (float)x.aln_span / (float)seq_len : 0.f;
        }
        ++n_pass;
    }
    if (n_pass == 0 || aln_len_at_best == 0 || g.best <= 0) {           // :1071-1083
        if (n_mapped_in == 0) { c.no_mapping += 1; g.verdict = kGroupNoMapping; }
        else { c.no_valid_aln += 1; g.verdict = kGroupNoValidAln; }
        return g;
    }
    if (aln_frac_at_best < F.min_aligned_fraction) {                    // :1084-1089
        c.discard_aln_frac += 1;
        g.verdict = kGroupAlnFrac;
        return g;
    }
    c.valid_best_aln += 1;                                              // :1092
    g.verdict = kGroupValid;
    const float inv_max_score = 1.0f / (float)g.best;                   // :1095-1096
    for (uint32_t i = 0; i < n; ++i) {                                  // :1107-1118
        const oem_aln_record &x = ag[i];
        if (filter_record(F, x, txp_len, n_txps) != kFilterPass) continue;
        if (filter_score_ok(F, x, inv_max_score)) g.n_kept += 1;
        else c.discard_score += 1;
    }
    return g;
}

// The second walk again, for a group whose verdict is kGroupValid: emit(k, i, x, gap) for the k-th retained record,
// record i of the group.
template <typename Emit>
OEM_HD inline void filter_group_emit(const oem_filters &F, const oem_aln_record *ag, uint32_t n, const uint64_t *txp_len,
                                     uint32_t n_txps, int32_t best, Emit &&emit)
{
    const float inv_max_score = 1.0f / (float)best;
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const oem_aln_record &x = ag[i];
        if (filter_record(F, x, txp_len, n_txps) != kFilterPass) continue;
        if (!filter_score_ok(F, x, inv_max_score)) continue;
        emit(k++, i, x, filter_gap(best, x));
    }
}

// -- host only: the discard table, the gap table ---------------------------------------------------------------------------
void add_counts(oem_discard_table &dt, const FilterCounts &c); // oem_builder.cpp: a group's contributions into the table


// D admits the gap table at all (finite and positive)
inline bool filter_denom_ok(float D) { return D > 0.0f && D <= 3.4028234663852886e38f; }

// tab[g] = expf((float)(-g) / D), g = 0 .. the first g whose value is +0.0f, that entry included.  false (tab
// unspecified) when D does not admit a table or it would need more than kFilterTabMax entries.
inline bool filter_prob_table(float D, std::vector<float> &tab)
{
    tab.clear();
    if (!filter_denom_ok(D)) return false;
    if (expf((float)(-(int64_t)(kFilterTabMax - 1)) / D) != 0.0f) return false;
    for (uint64_t g = 0; g < kFilterTabMax; ++g) {
        const float v = expf((float)(-(int64_t)g) / D);
        tab.push_back(v);
        if (v == 0.0f) return true;
    }
    return false;
}

} // namespace oem
