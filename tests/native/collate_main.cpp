// Stand-alone host program over oarfish_amd/csrc/oem_collate.h (tests/test_collate.py builds it with the address and
// undefined-behaviour sanitizers).  Cases on stdin, one answer line each:
//   C mode n_records n_cells has_secondary
//   cell_rec_off_0 .. cell_rec_off_{n_cells}
//   then n_records lines  name_as_hex secondary     ("-" for an empty name)
//       -> ok n_groups | order | group_off (n_groups + 1) | cell_group_off (n_cells + 1)
//       or bad record zero_byte
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../oarfish_amd/csrc/oem_collate.h"

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

int main()
{
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] != 'C') return 2;
        uint32_t mode, n_cells, has_sec;
        uint64_t n;
        if (scanf("%" SCNu32 " %" SCNu64 " %" SCNu32 " %" SCNu32, &mode, &n, &n_cells, &has_sec) != 4) return 2;
        std::vector<uint64_t> cell_rec_off(n_cells + 1);
        for (auto &v : cell_rec_off)
            if (scanf("%" SCNu64, &v) != 1) return 2;
        // exactly the bytes of the names: one read past them is a sanitizer report
        std::vector<uint8_t> blob, sec(n);
        std::vector<uint64_t> off(n + 1, 0);
        for (uint64_t i = 0; i < n; ++i) {
            char hex[1024];
            uint32_t s;
            if (scanf("%1023s %" SCNu32, hex, &s) != 2) return 2;
            if (hex[0] != '-')
                for (size_t k = 0; hex[k] && hex[k + 1]; k += 2) blob.push_back((uint8_t)(hexval(hex[k]) * 16 + hexval(hex[k + 1])));
            off[i + 1] = blob.size();
            sec[i] = (uint8_t)s;
        }
        std::vector<uint32_t> order(n);
        std::vector<uint64_t> group_off(n + 1), cell_group_off(n_cells + 1);
        uint64_t n_groups = 0;
        bool zero_byte = false;
        const uint64_t bad = oem::collate_host(blob.data(), off.data(), has_sec ? sec.data() : nullptr, n, cell_rec_off.data(), n_cells, mode,
                                               order.data(), group_off.data(), &n_groups, cell_group_off.data(), &zero_byte);
        if (bad != oem::kCollateNoRecord) {
            printf("bad %" PRIu64 " %d\n", bad, zero_byte ? 1 : 0);
            continue;
        }
        printf("ok %" PRIu64 " |", n_groups);
        for (uint64_t i = 0; i < n; ++i) printf(" %" PRIu32, order[i]);
        printf(" |");
        for (uint64_t g = 0; g <= n_groups; ++g) printf(" %" PRIu64, group_off[g]);
        printf(" |");
        for (uint32_t c = 0; c <= n_cells; ++c) printf(" %" PRIu64, cell_group_off[c]);
        putchar('\n');
    }
    return 0;
}
