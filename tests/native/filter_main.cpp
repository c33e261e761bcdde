// Stand-alone host program over oarfish_amd/csrc/oem_filter.h (tests/test_filter_groups.py builds it with the address and
// undefined-behaviour sanitizers).  Requests on stdin, one answer line each:
//   F five_prime_clip three_prime_clip score_threshold_bits min_aligned_fraction_bits min_aligned_len which_strand D_bits
//   T n len_0 .. len_{n-1}
//   G n  followed by n lines  ref_id aln_start aln_end aln_span score seq_len flags
//       -> verdict n_kept best flags bad_record | the ten counters | i:gap of every retained record
//   P D_bits   -> n followed by the table's entries as hex bit patterns (n = 0: no table for this D)
// (F and T answer "ok").  Floats travel as the hex bit patterns of their f32 values.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../oarfish_amd/csrc/oem_filter.h"

static float f32_of(uint32_t bits)
{
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

int main()
{
    oem_filters F;
    memset(&F, 0, sizeof(F));
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
        } else if (cmd[0] == 'T') {
            size_t n;
            if (scanf("%zu", &n) != 1) return 2;
            txp_len.assign(n, 0);
            for (size_t i = 0; i < n; ++i)
                if (scanf("%" SCNu64, &txp_len[i]) != 1) return 2;
            puts("ok");
        } else if (cmd[0] == 'G') {
            size_t n;
            if (scanf("%zu", &n) != 1) return 2;
            std::vector<oem_aln_record> ag(n); // exactly n records: one read past them is a sanitizer report
            for (size_t i = 0; i < n; ++i) {
                memset(&ag[i], 0, sizeof(ag[i]));
                if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNd64 " %" SCNd64 " %" SCNu32, &ag[i].ref_id,
                          &ag[i].aln_start, &ag[i].aln_end, &ag[i].aln_span, &ag[i].score, &ag[i].seq_len, &ag[i].flags) != 7)
                    return 2;
            }
            oem::FilterCounts c;
            const oem::FilterGroup g = oem::filter_group_measure(F, ag.data(), (uint32_t)n, txp_len.data(), (uint32_t)txp_len.size(), c);
            printf("%u %u %d %u %u |", g.verdict, g.n_kept, g.best, g.flags, g.bad_record);
            const uint32_t *cv = &c.discard_5p;
            for (int k = 0; k < oem::kFilterCounters; ++k) printf(" %u", cv[k]);
            printf(" |");
            if (g.verdict == oem::kGroupValid && !g.flags)
                oem::filter_group_emit(F, ag.data(), (uint32_t)n, txp_len.data(), (uint32_t)txp_len.size(), g.best,
                                       [](uint32_t, uint32_t i, const oem_aln_record &, uint64_t gap) { printf(" %u:%" PRIu64, i, gap); });
            putchar('\n');
        } else if (cmd[0] == 'P') {
            uint32_t d;
            if (scanf("%" SCNx32, &d) != 1) return 2;
            std::vector<float> tab;
            if (!oem::filter_prob_table(f32_of(d), tab)) tab.clear();
            printf("%zu", tab.size());
            for (float v : tab) {
                uint32_t b;
                memcpy(&b, &v, 4);
                printf(" %x", b);
            }
            putchar('\n');
        } else {
            return 2;
        }
    }
    return 0;
}
