// Stand-alone host program over the UMI rule of oarfish_amd/csrc/oem_collate.h (tests/test_dedup_umis.py builds it with
// the address and undefined-behaviour sanitizers).  Cases on stdin, one answer line each:
//   D n_records n_positions n_groups n_cells has_flags
//   then n_records lines  umi_as_hex flags        ("-" for an empty UMI)
//   then the n_positions entries of order, the n_groups + 1 of group_off, the n_cells + 1 of cell_group_off
//       -> ok | dup | survivor | cell_dups | order' | group_off' | cell_group_off' | cell_rec_off'
//       or bad record
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
        if (cmd[0] != 'D') return 2;
        uint64_t n, m, ng, nc;
        int has_flags;
        if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %d", &n, &m, &ng, &nc, &has_flags) != 5) return 2;
        // exactly the bytes of the UMIs and exactly the entries of every array: one read past them is a sanitizer report
        std::vector<uint8_t> blob;
        std::vector<uint64_t> off(n + 1, 0), goff(ng + 1), cgo(nc + 1);
        std::vector<uint32_t> flags(n), order(m);
        for (uint64_t i = 0; i < n; ++i) {
            char hex[1024];
            if (scanf("%1023s %" SCNu32, hex, &flags[i]) != 2) return 2;
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
        const uint64_t bad = oem::dedup_first_bad_umi(blob.data(), off.data(), n);
        if (bad != oem::kCollateNoRecord) {
            printf("bad %" PRIu64 "\n", bad);
            continue;
        }
        std::vector<uint8_t> dup(ng);
        std::vector<uint64_t> survivor(ng), cell_dups(nc);
        oem::dedup_umis_host(blob.data(), off.data(), has_flags ? flags.data() : nullptr, order.data(), goff.data(), ng, cgo.data(), (uint32_t)nc,
                             dup.data(), survivor.data(), cell_dups.data());
        uint64_t n_dups = 0, removed = 0;
        for (uint64_t g = 0; g < ng; ++g)
            if (dup[g]) {
                ++n_dups;
                removed += goff[g + 1] - goff[g];
            }
        // the outputs of the drop at their exact sizes
        std::vector<uint32_t> order2(m - removed);
        std::vector<uint64_t> goff2(ng - n_dups + 1), cgo2(nc + 1), cro2(nc + 1);
        const uint64_t ng2 = oem::dedup_drop_host(order.data(), goff.data(), ng, cgo.data(), (uint32_t)nc, dup.data(), order2.data(), goff2.data(),
                                                  cgo2.data(), cro2.data());
        if (ng2 != ng - n_dups) return 3;
        printf("ok");
        put(dup, ng);
        put(survivor, ng);
        put(cell_dups, nc);
        put(order2, order2.size());
        put(goff2, goff2.size());
        put(cgo2, cgo2.size());
        put(cro2, cro2.size());
        putchar('\n');
    }
    return 0;
}
