// Stand-alone host program that holds the streamed any-order cell rule of oarfish_amd/csrc/oem_collate.h
// (ParseCellsAnyOrderStream, with the host form of the barcode table of oem_barcode_table.h) to the barcode rule's host
// walk on the survivors (collate_barcodes_host).  tests/test_cells_barcodes_any_order_stream.py builds it with the address
// and undefined-behaviour sanitizers.
//
//   parse_cells_any_order_main            one input on stdin:
//                                           n_records
//                                           then n_records lines  flags barcode_as_hex     ("-" for an empty barcode)
//     EVERY cutting of it -- each subset of the n - 1 inner record positions -- is pushed batch by batch from copies of
//     exactly the batch's size (one read past a batch, or one look at an unmapped record's bytes past them, is a
//     sanitizer report), under four tables: the default one, and a first capacity of 2 with the hash masked to 0 bits, to
//     2 bits and not at all.  Under the two masked tables the cutting of one record per batch must see a probe wrap
//     past the table's end and at least three rebuilds.  Prints
//       ok <cuttings> <n_cells> <n_unmapped> | cell_rec_off | labels as hex | order (positions among the survivors) |
//          survivors | rebuilds of the four tables at one record per batch
//     or  differs <what> <table> <cutting as a bit mask>.
//   parse_cells_any_order_main random <seed> <rounds>
//     seeded random inputs (up to 48 records over 9 barcodes of 1 to 17 bytes that share prefixes, a fifth unmapped
//     with bytes no survivor may carry) under random cuttings and random tables.  Prints  ok <rounds> <records>.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "oarfish_em.h"

#include "../../oarfish_amd/csrc/oem_collate.h"

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

struct Input {
    std::vector<oem_aln_record> rec;
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off{0};
    void add(uint32_t flags, const uint8_t *p, size_t len)
    {
        oem_aln_record r;
        memset(&r, 0, sizeof r);
        r.flags = flags;
        rec.push_back(r);
        blob.insert(blob.end(), p, p + len);
        off.push_back(blob.size());
    }
    uint64_t n() const { return rec.size(); }
};

struct Table {
    uint64_t slots0;
    uint32_t bits;
};
static const Table kTables[4] = {{oem::kBarcodeTableSlots0, 64}, {2, 0}, {2, 2}, {2, 64}};

// what the rule gives on the whole input: the barcode rule's host walk on the survivors
struct Expected {
    std::vector<uint64_t> survivors, cell_rec_off, order;
    std::vector<std::vector<uint8_t>> labels;
    uint64_t n_unmapped = 0;
};

static Expected expected_of(const Input &in)
{
    Expected e;
    std::vector<uint8_t> dense;
    std::vector<uint64_t> doff{0};
    for (uint64_t i = 0; i < in.n(); ++i) {
        if (in.rec[i].flags & OEM_REC_UNMAPPED) {
            ++e.n_unmapped;
            continue;
        }
        e.survivors.push_back(i);
        dense.insert(dense.end(), in.blob.begin() + in.off[i], in.blob.begin() + in.off[i + 1]);
        doff.push_back(dense.size());
    }
    const uint64_t m = e.survivors.size();
    std::vector<uint32_t> order(m);
    std::vector<uint64_t> cro(m + 1, 0);
    uint64_t nc = 0;
    bool zero = false;
    if (oem::collate_barcodes_host(dense.data(), doff.data(), m, order.data(), cro.data(), &nc, &zero) != oem::kCollateNoRecord) exit(3);
    e.order.assign(order.begin(), order.end());
    e.cell_rec_off.assign(cro.begin(), cro.begin() + nc + 1);
    for (uint64_t c = 0; c < nc; ++c) {
        const uint64_t k = order[cro[c]];
        e.labels.emplace_back(dense.begin() + doff[k], dense.begin() + doff[k + 1]);
    }
    return e;
}

static oem::ParseCellsAnyOrderStream run(const Input &in, const std::vector<uint64_t> &edges, const Table &t)
{
    oem::ParseCellsAnyOrderStream st(t.slots0, t.bits);
    for (size_t k = 0; k + 1 < edges.size(); ++k) {
        const uint64_t a = edges[k], b = edges[k + 1];
        std::vector<oem_aln_record> r(in.rec.begin() + a, in.rec.begin() + b);
        std::vector<uint8_t> bc(in.blob.begin() + in.off[a], in.blob.begin() + in.off[b]);
        std::vector<uint64_t> o(b - a + 1);
        for (uint64_t i = a; i <= b; ++i) o[i - a] = in.off[i] - in.off[a];
        st.push(r.data(), b - a, bc.data(), o.data());
    }
    st.finish();
    return st;
}

static const char *differs(const oem::ParseCellsAnyOrderStream &st, const Expected &e, uint64_t n)
{
    if (st.table.broken) return "table";
    if (st.cell_rec_off != e.cell_rec_off) return "cell_rec_off";
    if (st.order != e.order) return "order";
    if (st.survivors != e.survivors) return "survivors";
    if (st.n_unmapped != e.n_unmapped || st.n_records != n) return "counts";
    if (st.n_cells() != e.labels.size()) return "n_cells";
    for (uint64_t c = 0; c < st.n_cells(); ++c) {
        const std::vector<uint8_t> lab(st.table.labels.begin() + st.table.label_off[c], st.table.labels.begin() + st.table.label_off[c + 1]);
        if (lab != e.labels[c]) return "labels";
    }
    if (st.misses < st.n_cells() || st.misses > st.survivors.size()) return "misses";
    if (2 * st.n_cells() > st.table.slot.size()) return "load";
    return nullptr;
}

static int random_rounds(uint64_t seed, uint64_t rounds)
{
    uint64_t x = seed * 0x9e3779b97f4a7c15ull + 1;
    auto next = [&](uint64_t mod) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return (x >> 11) % mod;
    };
    const char *pool[9] = {"A", "AC", "ACGTACGT", "ACGTACGTA", "ACGTACGTC", "ACGTACGTACGTACGT", "ACGTACGTACGTACGT-", "T", "ACGTACGTACGTACGA"};
    const uint8_t garbage[2] = {0x00, 0xff};
    uint64_t records = 0;
    for (uint64_t r = 0; r < rounds; ++r) {
        Input in;
        const uint64_t n = 1 + next(48), kinds = 1 + next(9);
        for (uint64_t i = 0; i < n; ++i) {
            if (next(5) == 0) {
                in.add(OEM_REC_UNMAPPED, garbage, next(3));
            } else {
                const char *b = pool[next(kinds)];
                in.add(0, (const uint8_t *)b, strlen(b));
            }
        }
        const Expected e = expected_of(in);
        std::vector<uint64_t> edges{0};
        for (uint64_t p = 1; p < n; ++p)
            if (next(3) == 0) edges.push_back(p);
        if (next(4) == 0) edges.push_back(edges.back()); // an empty batch
        edges.push_back(n);
        const Table t = kTables[next(4)];
        const char *what = differs(run(in, edges, t), e, n);
        if (what) {
            printf("differs %s round %" PRIu64 "\n", what, r);
            return 1;
        }
        records += n;
    }
    printf("ok %" PRIu64 " %" PRIu64 "\n", rounds, records);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "random")) return random_rounds(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    uint64_t n;
    if (scanf("%" SCNu64, &n) != 1 || n < 1 || n > 20) return 2;
    Input in;
    for (uint64_t i = 0; i < n; ++i) {
        char hex[1024];
        uint32_t flags;
        if (scanf("%" SCNu32 " %1023s", &flags, hex) != 2) return 2;
        std::vector<uint8_t> b;
        if (hex[0] != '-')
            for (size_t k = 0; hex[k] && hex[k + 1]; k += 2) b.push_back((uint8_t)(hexval(hex[k]) * 16 + hexval(hex[k + 1])));
        in.add(flags, b.data(), b.size());
    }
    const Expected e = expected_of(in);
    uint64_t cuttings = 0, rebuilds[4] = {0, 0, 0, 0};
    for (uint64_t mask = 0; mask < (1ull << (n - 1)); ++mask, ++cuttings) {
        std::vector<uint64_t> edges{0};
        for (uint64_t p = 1; p < n; ++p)
            if (mask >> (p - 1) & 1) edges.push_back(p);
        edges.push_back(n);
        for (int t = 0; t < 4; ++t) {
            const oem::ParseCellsAnyOrderStream st = run(in, edges, kTables[t]);
            const char *what = differs(st, e, n);
            if (what) {
                printf("differs %s %d %" PRIu64 "\n", what, t, mask);
                return 1;
            }
            if (mask + 1 == (1ull << (n - 1))) { // one record per batch
                rebuilds[t] = st.table.rebuilds;
                if ((t == 1 || t == 2) && (!st.table.wrapped || st.table.rebuilds < 3)) {
                    printf("differs masked-table %d wrapped %d rebuilds %" PRIu64 "\n", t, (int)st.table.wrapped, st.table.rebuilds);
                    return 1;
                }
            }
        }
    }
    printf("ok %" PRIu64 " %zu %" PRIu64 " |", cuttings, e.labels.size(), e.n_unmapped);
    for (uint64_t v : e.cell_rec_off) printf(" %" PRIu64, v);
    printf(" |");
    for (const auto &b : e.labels) {
        putchar(' ');
        for (uint8_t c : b) printf("%02x", c);
    }
    printf(" |");
    for (uint64_t v : e.order) printf(" %" PRIu64, v);
    printf(" |");
    for (uint64_t v : e.survivors) printf(" %" PRIu64, v);
    printf(" |");
    for (uint64_t v : rebuilds) printf(" %" PRIu64, v);
    putchar('\n');
    return 0;
}
