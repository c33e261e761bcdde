// Stand-alone host program that holds the streamed bulk rule of oarfish_amd/csrc/oem_collate.h (ParseBulkStream) to
// parse_bulk_host on the concatenation (tests/test_records_stream_names.py builds it with the address and
// undefined-behaviour sanitizers).  One input on stdin:
//   n_records
//   then n_records lines  flags name_as_hex     ("-" for an empty name)
// Every cutting of it is pushed batch by batch from copies of exactly the batch's size -- one read past a batch is a
// sanitizer report: no cut, every single cut (n + 1 positions), every pair of distinct cuts, and one record per batch.
// Prints  ok <cuttings> <n_groups> <n_unmapped> | sizes | heads   or  differs <what> <cut a> <cut b>.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "oarfish_em.h"

#include "../../oarfish_amd/csrc/oem_collate.h"

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

int main()
{
    uint64_t n;
    if (scanf("%" SCNu64, &n) != 1) return 2;
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off(n + 1, 0);
    std::vector<oem_aln_record> rec(n);
    for (uint64_t i = 0; i < n; ++i) {
        char hex[1024];
        uint32_t flags;
        if (scanf("%" SCNu32 " %1023s", &flags, hex) != 2) return 2;
        memset(&rec[i], 0, sizeof rec[i]);
        rec[i].flags = flags;
        if (hex[0] != '-')
            for (size_t k = 0; hex[k] && hex[k + 1]; k += 2) blob.push_back((uint8_t)(hexval(hex[k]) * 16 + hexval(hex[k + 1])));
        off[i + 1] = blob.size();
    }
    std::vector<uint32_t> order(n);
    std::vector<uint64_t> group_off(n + 1);
    const oem::ParseBulk pb =
        oem::parse_bulk_host(rec.data(), n, blob.data(), off.data(), (const uint8_t *)nullptr, oem::kCollateAdjacent, 0, order.data(), group_off.data());
    if (pb.bad_record != oem::kCollateNoRecord) return 3;
    std::vector<uint64_t> size(pb.n_groups), head(pb.n_groups);
    for (uint64_t g = 0; g < pb.n_groups; ++g) {
        size[g] = group_off[g + 1] - group_off[g];
        head[g] = order[group_off[g]];
    }

    auto run = [&](const std::vector<uint64_t> &edges) -> const char * { // edges: 0 ... n, ascending
        oem::ParseBulkStream st;
        for (size_t k = 0; k + 1 < edges.size(); ++k) {
            const uint64_t a = edges[k], b = edges[k + 1];
            std::vector<oem_aln_record> r(rec.begin() + a, rec.begin() + b);
            std::vector<uint8_t> nm(blob.begin() + off[a], blob.begin() + off[b]);
            std::vector<uint64_t> o(b - a + 1);
            for (uint64_t i = a; i <= b; ++i) o[i - a] = off[i] - off[a];
            st.push(r.data(), b - a, nm.data(), o.data());
        }
        st.finish();
        if (st.group_size != size) return "sizes";
        if (st.group_head != head) return "heads";
        if (st.n_unmapped != pb.n_unmapped) return "n_unmapped";
        if (st.n_records != n) return "n_records";
        return nullptr;
    };
    uint64_t cuttings = 0;
    auto hold = [&](const std::vector<uint64_t> &edges, uint64_t a, uint64_t b) {
        ++cuttings;
        const char *what = run(edges);
        if (what) printf("differs %s %" PRIu64 " %" PRIu64 "\n", what, a, b);
        return what == nullptr;
    };
    for (uint64_t a = 0; a <= n; ++a)
        if (!hold({0, a, n}, a, a)) return 1;
    for (uint64_t a = 0; a <= n; ++a)
        for (uint64_t b = a + 1; b <= n; ++b)
            if (!hold({0, a, b, n}, a, b)) return 1;
    std::vector<uint64_t> each;
    for (uint64_t i = 0; i <= n; ++i) each.push_back(i);
    if (!hold(each, n, n)) return 1;
    printf("ok %" PRIu64 " %" PRIu64 " %" PRIu64 " |", cuttings, pb.n_groups, pb.n_unmapped);
    for (uint64_t g = 0; g < pb.n_groups; ++g) printf(" %" PRIu64, size[g]);
    printf(" |");
    for (uint64_t g = 0; g < pb.n_groups; ++g) printf(" %" PRIu64, head[g]);
    putchar('\n');
    return 0;
}
