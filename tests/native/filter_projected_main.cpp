// Stand-alone host program over oarfish_amd/csrc/oem_filter_projected.h and oem_exp_f32.h (tests/test_filter_projected.py
// builds it with the address and undefined-behaviour sanitizers).  Requests on stdin, one answer line each:
//   F five_prime_clip three_prime_clip score_threshold_bits min_aligned_fraction_bits min_aligned_len which_strand D_bits
//   O beta_bits prob_source
//   T n len_0 .. len_{n-1}
//   G n read_len  followed by n lines  ref_id start end aligned_len query_aligned_len aln_score flags similarity_bits
//       -> verdict n_kept best_sim_bits best_score flags bad_record | the ten counters | i:start:end:f_bits of every kept record
//   X f_bits      -> candidate_bits sure expf_bits
//   S first_bits last_bits stride   the f32 whose bit patterns are first, first + stride, .. <= last
//       -> n  n_unsure  n_sure_that_differ_from_expf  n_candidates_that_differ_from_expf
// (F, O and T answer "ok").  f32 travel as hex bit patterns of 32 bits, f64 of 64.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../oarfish_amd/csrc/oem_exp_f32.h"
#include "../../oarfish_amd/csrc/oem_filter_projected.h"

static float f32_of(uint32_t bits)
{
    float f;
    memcpy(&f, &bits, 4);
    return f;
}
static uint32_t bits_of(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

int main()
{
    oem_filters F;
    memset(&F, 0, sizeof(F));
    oem_proj_opts P = {10.0f, OEM_PROJ_SIMILARITY};
    std::vector<uint64_t> txp_len;
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'F') {
            uint32_t thr, frac, d;
            if (scanf("%" SCNu32 " %" SCNd64 " %" SCNx32 " %" SCNx32 " %" SCNu32 " %" SCNd32 " %" SCNx32, &F.five_prime_clip,
                      &F.three_prime_clip, &thr, &frac, &F.min_aligned_len, &F.which_strand, &d) != 7) return 2;
            F.score_threshold = f32_of(thr);
            F.min_aligned_fraction = f32_of(frac);
            F.score_prob_denom = f32_of(d);
            puts("ok");
        } else if (cmd[0] == 'O') {
            uint32_t beta;
            if (scanf("%" SCNx32 " %" SCNd32, &beta, &P.prob_source) != 2 || !oem::proj_source_ok(P.prob_source)) return 2;
            P.beta = f32_of(beta);
            puts("ok");
        } else if (cmd[0] == 'T') {
            size_t n;
            if (scanf("%zu", &n) != 1) return 2;
            txp_len.assign(n, 0);
            for (size_t i = 0; i < n; ++i)
                if (scanf("%" SCNu64, &txp_len[i]) != 1) return 2;
            puts("ok");
        } else if (cmd[0] == 'G') {
            size_t n;
            uint64_t read_len;
            if (scanf("%zu %" SCNu64, &n, &read_len) != 2) return 2;
            std::vector<oem_proj_record> ag(n); // exactly n records: one read past them is a sanitizer report
            for (size_t i = 0; i < n; ++i) {
                memset(&ag[i], 0, sizeof(ag[i]));
                uint64_t sim;
                if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNd32 " %" SCNu32 " %" SCNx64, &ag[i].ref_id,
                          &ag[i].start, &ag[i].end, &ag[i].aligned_len, &ag[i].query_aligned_len, &ag[i].aln_score, &ag[i].flags,
                          &sim) != 8)
                    return 2;
                memcpy(&ag[i].similarity, &sim, 8);
            }
            const uint32_t T = (uint32_t)txp_len.size();
            oem::FilterCounts c;
            const oem::ProjGroup g = oem::proj_group_measure(F, ag.data(), (uint32_t)n, read_len, txp_len.data(), T, c);
            uint64_t best;
            memcpy(&best, &g.best_sim, 8);
            printf("%u %u %" PRIx64 " %d %u %u |", g.verdict, g.n_kept, best, g.best_score, g.flags, g.bad_record);
            const uint32_t *cv = &c.discard_5p;
            for (int k = 0; k < oem::kFilterCounters; ++k) printf(" %u", cv[k]);
            printf(" |");
            if (g.verdict == oem::kProjValid && !(g.flags & oem::kFilterFlagBadRef))
                oem::proj_group_emit(F, P, ag.data(), (uint32_t)n, txp_len.data(), T, g.best_sim, g.best_score,
                                     [](uint32_t, uint32_t i, const oem_proj_record &, uint32_t s, uint32_t e, float f) {
                                         printf(" %u:%u:%u:%x", i, s, e, bits_of(f));
                                     });
            putchar('\n');
        } else if (cmd[0] == 'X') {
            uint32_t b;
            if (scanf("%" SCNx32, &b) != 1) return 2;
            bool sure;
            const float c = oem::exp_f32_candidate(f32_of(b), &sure);
            printf("%x %d %x\n", bits_of(c), sure ? 1 : 0, bits_of(expf(f32_of(b))));
        } else if (cmd[0] == 'S') {
            uint32_t first, last, stride;
            if (scanf("%" SCNx32 " %" SCNx32 " %" SCNu32, &first, &last, &stride) != 3 || stride == 0 || last < first) return 2;
            uint64_t n = 0, n_unsure = 0, n_sure_bad = 0, n_cand_bad = 0;
            for (uint64_t b = first; b <= last; b += stride) {
                const float f = f32_of((uint32_t)b);
                bool sure;
                const uint32_t c = bits_of(oem::exp_f32_candidate(f, &sure)), want = bits_of(expf(f));
                ++n;
                if (!sure) ++n_unsure;
                if (c != want) ++n_cand_bad;
                if (sure && c != want) ++n_sure_bad;
            }
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", n, n_unsure, n_sure_bad, n_cand_bad);
        } else {
            return 2;
        }
    }
    return 0;
}
