// Stand-alone host program that holds the streamed cell rule of oarfish_amd/csrc/oem_collate.h (ParseCellsStream) to
// its own uncut walk (tests/test_cells_barcodes_stream.py builds it with the address and undefined-behaviour
// sanitizers).  One input on stdin:
//   n_records
//   then n_records lines  flags barcode_as_hex     ("-" for an empty barcode)
// EVERY cutting of it -- each subset of the n - 1 inner record positions -- is pushed batch by batch from copies of
// exactly the batch's size: one read past a batch, or one look at an unmapped record's bytes past them, is a sanitizer
// report.  Prints  ok <cuttings> <n_cells> <n_unmapped> | cell_rec_off | labels as hex | survivors   or
// differs <what> <cutting as a bit mask>.
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
    if (scanf("%" SCNu64, &n) != 1 || n < 1 || n > 20) return 2;
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
    auto run = [&](const std::vector<uint64_t> &edges) { // edges: 0 ... n, ascending
        oem::ParseCellsStream st;
        for (size_t k = 0; k + 1 < edges.size(); ++k) {
            const uint64_t a = edges[k], b = edges[k + 1];
            std::vector<oem_aln_record> r(rec.begin() + a, rec.begin() + b);
            std::vector<uint8_t> bc(blob.begin() + off[a], blob.begin() + off[b]);
            std::vector<uint64_t> o(b - a + 1);
            for (uint64_t i = a; i <= b; ++i) o[i - a] = off[i] - off[a];
            st.push(r.data(), b - a, bc.data(), o.data());
        }
        st.finish();
        return st;
    };
    const oem::ParseCellsStream whole = run({0, n});
    uint64_t cuttings = 0;
    for (uint64_t mask = 0; mask < (1ull << (n - 1)); ++mask, ++cuttings) {
        std::vector<uint64_t> edges{0};
        for (uint64_t p = 1; p < n; ++p)
            if (mask >> (p - 1) & 1) edges.push_back(p);
        edges.push_back(n);
        const oem::ParseCellsStream st = run(edges);
        const char *what = st.cell_rec_off != whole.cell_rec_off   ? "cell_rec_off"
                           : st.cell_barcode != whole.cell_barcode ? "labels"
                           : st.survivors != whole.survivors       ? "survivors"
                           : st.n_unmapped != whole.n_unmapped     ? "n_unmapped"
                           : st.n_records != n || st.open          ? "state"
                                                                   : nullptr;
        if (what) {
            printf("differs %s %" PRIu64 "\n", what, mask);
            return 1;
        }
    }
    printf("ok %" PRIu64 " %zu %" PRIu64 " |", cuttings, whole.cell_barcode.size(), whole.n_unmapped);
    for (uint64_t v : whole.cell_rec_off) printf(" %" PRIu64, v);
    printf(" |");
    for (const auto &b : whole.cell_barcode) {
        putchar(' ');
        for (uint8_t c : b) printf("%02x", c);
    }
    printf(" |");
    for (uint64_t v : whole.survivors) printf(" %" PRIu64, v);
    putchar('\n');
    return 0;
}
