// Stand-alone host program over the bulk parser's rule of oarfish_amd/csrc/oem_collate.h (tests/test_parse_names.py
// builds it with the address and undefined-behaviour sanitizers).  Cases on stdin, one answer line each:
//   P n_records mode sort_check_num
//   then n_records lines  flags secondary name_as_hex     ("-" for an empty name)
//       -> ok n_unmapped n_parsed n_groups n_checked | order | group_off (n_groups + 1)
//       or bad record zero_byte
//       or repeat group record earlier_record n_unmapped n_parsed n_groups n_checked | order | group_off
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "oarfish_em.h"

#include "../../oarfish_amd/csrc/oem_collate.h"

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

int main()
{
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] != 'P') return 2;
        uint64_t n, check;
        uint32_t mode;
        if (scanf("%" SCNu64 " %" SCNu32 " %" SCNu64, &n, &mode, &check) != 3) return 2;
        // exactly the bytes of the names and exactly n records: one read past them is a sanitizer report
        std::vector<uint8_t> blob, sec(n);
        std::vector<uint64_t> off(n + 1, 0);
        std::vector<oem_aln_record> rec(n);
        for (uint64_t i = 0; i < n; ++i) {
            char hex[1024];
            uint32_t flags, s;
            if (scanf("%" SCNu32 " %" SCNu32 " %1023s", &flags, &s, hex) != 3) return 2;
            memset(&rec[i], 0, sizeof rec[i]);
            rec[i].flags = flags;
            sec[i] = (uint8_t)s;
            if (hex[0] != '-')
                for (size_t k = 0; hex[k] && hex[k + 1]; k += 2) blob.push_back((uint8_t)(hexval(hex[k]) * 16 + hexval(hex[k + 1])));
            off[i + 1] = blob.size();
        }
        std::vector<uint32_t> order(n);
        std::vector<uint64_t> group_off(n + 1);
        const oem::ParseBulk pb =
            oem::parse_bulk_host(rec.data(), n, blob.data(), off.data(), sec.data(), mode, check, order.data(), group_off.data());
        if (pb.bad_record != oem::kCollateNoRecord) {
            printf("bad %" PRIu64 " %d\n", pb.bad_record, pb.zero_byte ? 1 : 0);
            continue;
        }
        if (pb.repeat_group != oem::kCollateNoRecord)
            printf("repeat %" PRIu64 " %" PRIu64 " %" PRIu64, pb.repeat_group, pb.repeat_record, pb.earlier_record);
        else
            printf("ok");
        printf(" %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " |", pb.n_unmapped, pb.n_parsed, pb.n_groups, pb.n_checked);
        for (uint64_t i = 0; i < pb.n_parsed; ++i) printf(" %" PRIu32, order[i]);
        printf(" |");
        for (uint64_t g = 0; g <= pb.n_groups; ++g) printf(" %" PRIu64, group_off[g]);
        putchar('\n');
    }
    return 0;
}
