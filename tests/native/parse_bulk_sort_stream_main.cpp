// Stand-alone host program that holds the streamed sort rule of oarfish_amd/csrc/oem_collate.h (ParseBulkSortStream) to
// parse_bulk_host(kCollateSort) on the concatenation (tests/test_records_stream_sort.py builds it with the address and
// undefined-behaviour sanitizers).  One input on stdin:
//   n_records
//   then n_records lines  flags secondary name_as_hex     ("-" for an empty name)
// Every cutting of it is pushed batch by batch from copies of exactly the batch's size -- one read past a batch is a
// sanitizer report: every single cut (n + 1 positions), every pair of distinct cuts, and one record per batch; each
// once with the flags and once without (a batch pushed without flags counts as flags of 0).  Then <seed> <rounds> from
// the command line: that many random inputs (names over a small alphabet with long shared prefixes, unmapped records
// with bad names, a surviving bad name now and then, random flags) under random cuttings, some batches without flags.
// Prints  ok <cuttings> <n_groups> <n_unmapped> <random inputs> | order | group_off   or  differs <what> <a> <b>.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "oarfish_em.h"

#include "../../oarfish_amd/csrc/oem_collate.h"

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

struct Input {
    std::vector<oem_aln_record> rec;
    std::vector<uint8_t> blob, sec;
    std::vector<uint64_t> off{0};
    uint64_t n() const { return rec.size(); }
    void add(uint32_t flags, uint8_t secondary, const std::vector<uint8_t> &name)
    {
        oem_aln_record r;
        memset(&r, 0, sizeof r);
        r.flags = flags;
        rec.push_back(r);
        sec.push_back(secondary);
        blob.insert(blob.end(), name.begin(), name.end());
        off.push_back(blob.size());
    }
};

// The whole parse of the concatenation; with_sec[k]: batch k (edges[k] .. edges[k + 1]) was pushed with its flags.
struct Whole {
    oem::ParseBulk pb;
    std::vector<uint64_t> order, group_off;
};
static Whole whole(const Input &in, const std::vector<uint64_t> &edges, const std::vector<bool> &with_sec)
{
    const uint64_t n = in.n();
    std::vector<uint8_t> sec(n + 1, 0);
    for (size_t k = 0; k + 1 < edges.size(); ++k)
        for (uint64_t i = edges[k]; i < edges[k + 1]; ++i) sec[i] = with_sec[k] ? in.sec[i] : 0;
    std::vector<uint32_t> order(n + 1);
    std::vector<uint64_t> goff(n + 2);
    std::vector<uint8_t> blob(in.blob);
    blob.push_back(0);
    Whole w;
    w.pb = oem::parse_bulk_host(in.rec.data(), n, blob.data(), in.off.data(), sec.data(), oem::kCollateSort, 0, order.data(), goff.data());
    if (w.pb.bad_record == oem::kCollateNoRecord) {
        w.order.assign(order.begin(), order.begin() + w.pb.n_parsed);
        w.group_off.assign(goff.begin(), goff.begin() + w.pb.n_groups + 1);
    }
    return w;
}

static const char *run(const Input &in, const std::vector<uint64_t> &edges, const std::vector<bool> &with_sec, const Whole &w)
{
    oem::ParseBulkSortStream st;
    for (size_t k = 0; k + 1 < edges.size(); ++k) {
        const uint64_t a = edges[k], b = edges[k + 1];
        std::vector<oem_aln_record> r(in.rec.begin() + a, in.rec.begin() + b);
        std::vector<uint8_t> nm(in.blob.begin() + in.off[a], in.blob.begin() + in.off[b]);
        std::vector<uint8_t> sc(in.sec.begin() + a, in.sec.begin() + b);
        std::vector<uint64_t> o(b - a + 1);
        for (uint64_t i = a; i <= b; ++i) o[i - a] = in.off[i] - in.off[a];
        st.push(r.data(), b - a, nm.data(), o.data(), with_sec[k] ? sc.data() : (const uint8_t *)nullptr);
    }
    st.finish();
    if (st.n_records != in.n()) return "n_records";
    if (st.n_unmapped != w.pb.n_unmapped) return "n_unmapped";
    if (st.n_parsed() != w.pb.n_parsed) return "n_parsed";
    if (st.bad_record != w.pb.bad_record) return "bad_record";
    if (st.bad_record != oem::kCollateNoRecord) return st.zero_byte == w.pb.zero_byte ? nullptr : "zero_byte";
    if (st.order != w.order) return "order";
    if (w.pb.n_parsed && st.group_off != w.group_off) return "group_off";
    if (!w.pb.n_parsed && st.group_off != std::vector<uint64_t>{0}) return "group_off of nothing";
    return nullptr;
}

int main(int argc, char **argv)
{
    uint64_t n;
    if (scanf("%" SCNu64, &n) != 1) return 2;
    Input in;
    for (uint64_t i = 0; i < n; ++i) {
        char hex[1024];
        uint32_t flags, secondary;
        if (scanf("%" SCNu32 " %" SCNu32 " %1023s", &flags, &secondary, hex) != 3) return 2;
        std::vector<uint8_t> name;
        if (hex[0] != '-')
            for (size_t k = 0; hex[k] && hex[k + 1]; k += 2) name.push_back((uint8_t)(hexval(hex[k]) * 16 + hexval(hex[k + 1])));
        in.add(flags, (uint8_t)secondary, name);
    }
    uint64_t cuttings = 0;
    Whole first;
    auto hold = [&](const std::vector<uint64_t> &edges, uint64_t a, uint64_t b) {
        for (int flagged = 1; flagged >= 0; --flagged) {
            ++cuttings;
            const std::vector<bool> with_sec(edges.size(), flagged != 0);
            const Whole w = whole(in, edges, with_sec);
            if (cuttings == 1) first = w;
            if (flagged && (w.order != first.order || w.group_off != first.group_off)) {
                printf("differs the-whole-parse %" PRIu64 " %" PRIu64 "\n", a, b);
                return false;
            }
            const char *what = run(in, edges, with_sec, w);
            if (what) {
                printf("differs %s %" PRIu64 " %" PRIu64 "\n", what, a, b);
                return false;
            }
        }
        return true;
    };
    for (uint64_t a = 0; a <= n; ++a)
        if (!hold({0, a, n}, a, a)) return 1;
    for (uint64_t a = 0; a <= n; ++a)
        for (uint64_t b = a + 1; b <= n; ++b)
            if (!hold({0, a, b, n}, a, b)) return 1;
    std::vector<uint64_t> each;
    for (uint64_t i = 0; i <= n; ++i) each.push_back(i);
    if (!hold(each, n, n)) return 1;
    if (first.pb.bad_record != oem::kCollateNoRecord) return 3;

    // seeded random inputs
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1, rounds = argc > 2 ? strtoull(argv[2], nullptr, 10) : 0;
    std::mt19937_64 rng(seed);
    auto below = [&](uint64_t k) { return (uint64_t)(rng() % k); };
    for (uint64_t round = 0; round < rounds; ++round) {
        Input ri;
        const uint64_t rn = below(48), n_names = 1 + below(9);
        const bool plant_bad = below(8) == 0;
        for (uint64_t i = 0; i < rn; ++i) {
            const bool unmapped = below(5) == 0;
            std::vector<uint8_t> name;
            if (unmapped && below(2)) {
                if (below(2)) name = {'a', 0, 'b'}; // never read
            } else if (!unmapped && plant_bad && below(12) == 0) {
                if (below(2)) name = {'x', 0};
            } else { // 21 shared bytes, then a tail of 0 .. 3 bytes: several names are prefixes of others
                const uint64_t id = below(n_names);
                name.assign(21, (uint8_t)'P');
                for (uint64_t k = 0; k < id % 4; ++k) name.push_back((uint8_t)('a' + id / 4));
            }
            ri.add(unmapped ? oem::kRecUnmapped : 0u, (uint8_t)(below(3) == 0 ? 1 + below(200) : 0), name);
        }
        std::vector<uint64_t> edges{0};
        const uint64_t n_cuts = below(6);
        for (uint64_t k = 0; k < n_cuts; ++k) edges.push_back(below(rn + 1));
        edges.push_back(rn);
        std::sort(edges.begin(), edges.end());
        std::vector<bool> with_sec(edges.size());
        for (size_t k = 0; k < with_sec.size(); ++k) with_sec[k] = below(4) != 0;
        const Whole w = whole(ri, edges, with_sec);
        const char *what = run(ri, edges, with_sec, w);
        if (what) {
            printf("differs %s random %" PRIu64 "\n", what, round);
            return 1;
        }
    }
    printf("ok %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " |", cuttings, first.pb.n_groups, first.pb.n_unmapped, rounds);
    for (uint64_t v : first.order) printf(" %" PRIu64, v);
    printf(" |");
    for (uint64_t v : first.group_off) printf(" %" PRIu64, v);
    putchar('\n');
    return 0;
}
