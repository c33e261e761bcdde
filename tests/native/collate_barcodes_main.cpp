// Stand-alone host program over the barcode rule of oarfish_amd/csrc/oem_collate.h (tests/test_collate_barcodes.py builds
// it with the address and undefined-behaviour sanitizers).  Cases on stdin, one answer line each:
//   B n_records
//   then n_records lines  barcode_as_hex     ("-" for an empty barcode)
//       -> ok n_cells | order | cell_rec_off (n_cells + 1)
//       or bad record zero_byte
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../oarfish_amd/csrc/oem_collate.h"

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

int main()
{
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] != 'B') return 2;
        uint64_t n;
        if (scanf("%" SCNu64, &n) != 1) return 2;
        // exactly the bytes of the barcodes: one read past them is a sanitizer report
        std::vector<uint8_t> blob;
        std::vector<uint64_t> off(n + 1, 0);
        for (uint64_t i = 0; i < n; ++i) {
            char hex[1024];
            if (scanf("%1023s", hex) != 1) return 2;
            if (hex[0] != '-')
                for (size_t k = 0; hex[k] && hex[k + 1]; k += 2) blob.push_back((uint8_t)(hexval(hex[k]) * 16 + hexval(hex[k + 1])));
            off[i + 1] = blob.size();
        }
        std::vector<uint32_t> order(n);
        std::vector<uint64_t> cell_rec_off(n + 1);
        uint64_t n_cells = 0;
        bool zero_byte = false;
        const uint64_t bad = oem::collate_barcodes_host(blob.data(), off.data(), n, order.data(), cell_rec_off.data(), &n_cells, &zero_byte);
        if (bad != oem::kCollateNoRecord) {
            printf("bad %" PRIu64 " %d\n", bad, zero_byte ? 1 : 0);
            continue;
        }
        printf("ok %" PRIu64 " |", n_cells);
        for (uint64_t i = 0; i < n; ++i) printf(" %" PRIu32, order[i]);
        printf(" |");
        for (uint64_t c = 0; c <= n_cells; ++c) printf(" %" PRIu64, cell_rec_off[c]);
        putchar('\n');
    }
    return 0;
}
