// Stand-alone host program over the UMI rule (gene_of, correct) of oarfish_amd/csrc/oem_collate.h
// (tests/test_dedup_umis_rule.py builds it with the address and undefined-behaviour sanitizers).  Cases on stdin, one
// answer line each:
//   R n_records n_positions n_groups n_cells has_flags n_txps correct      (n_txps = 0: no gene_of)
//   then n_records lines  umi_as_hex flags ref_id        ("-" for an empty UMI)
//   then the n_positions entries of order, the n_groups + 1 of group_off, the n_cells + 1 of cell_group_off and the
//   n_txps entries of gene_of
//       -> ok | dup | survivor | cell_dups | cell_corrected
//       or bad record          (a UMI with a 0 byte)
//       or badref record       (the head of a read that takes part whose ref_id is not below n_txps)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../oarfish_amd/csrc/oem_collate.h"

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

template <typename V>
static void put(const V &v, size_t n)
{
    printf(" |");
    for (size_t i = 0; i < n; ++i) printf(" %" PRIu64, (uint64_t)v[i]);
}

int main()
{
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] != 'R') return 2;
        uint64_t n, m, ng, nc;
        int has_flags;
        uint32_t n_txps, correct;
        if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %d %" SCNu32 " %" SCNu32, &n, &m, &ng, &nc, &has_flags, &n_txps, &correct) != 7)
            return 2;
        // exactly the bytes of the UMIs and exactly the entries of every array: one read past them is a sanitizer report
        std::vector<uint8_t> blob;
        std::vector<uint64_t> off(n + 1, 0), goff(ng + 1), cgo(nc + 1);
        std::vector<uint32_t> flags(n), ref_id(n), order(m), gene_of(n_txps);
        for (uint64_t i = 0; i < n; ++i) {
            char hex[1024];
            if (scanf("%1023s %" SCNu32 " %" SCNu32, hex, &flags[i], &ref_id[i]) != 3) return 2;
            if (hex[0] != '-')
                for (size_t k = 0; hex[k] && hex[k + 1]; k += 2) blob.push_back((uint8_t)(hexval(hex[k]) * 16 + hexval(hex[k + 1])));
            off[i + 1] = blob.size();
        }
        for (auto &v : order)
            if (scanf("%" SCNu32, &v) != 1) return 2;
        for (auto &v : goff)
            if (scanf("%" SCNu64, &v) != 1) return 2;
        for (auto &v : cgo)
            if (scanf("%" SCNu64, &v) != 1) return 2;
        for (auto &v : gene_of)
            if (scanf("%" SCNu32, &v) != 1) return 2;
        uint64_t bad = oem::dedup_first_bad_umi(blob.data(), off.data(), n);
        if (bad != oem::kCollateNoRecord) {
            printf("bad %" PRIu64 "\n", bad);
            continue;
        }
        std::vector<uint8_t> dup(ng);
        std::vector<uint64_t> survivor(ng), cell_dups(nc), cell_corrected(nc);
        bad = oem::dedup_umis_rule_host(blob.data(), off.data(), has_flags ? flags.data() : nullptr, ref_id.data(),
                                        n_txps ? gene_of.data() : nullptr, n_txps, correct, order.data(), goff.data(), ng, cgo.data(),
                                        (uint32_t)nc, dup.data(), survivor.data(), cell_dups.data(), cell_corrected.data());
        if (bad != oem::kCollateNoRecord) {
            printf("badref %" PRIu64 "\n", bad);
            continue;
        }
        printf("ok");
        put(dup, ng);
        put(survivor, ng);
        put(cell_dups, nc);
        put(cell_corrected, nc);
        putchar('\n');
    }
    return 0;
}
