// Stand-alone host program over "UMIs in the sessions" of oarfish_amd/csrc/oem_collate.h (tests/test_cells_umis_stream.py
// builds it with the address and undefined-behaviour sanitizers): a session deduplicates GROUP BY GROUP, with
// group-local record indices and the group's window of the arena's UMI offsets, and joins the groups' pieces; this must
// be the whole-input walk whatever the groups are.  One input on stdin:
//   n_records
//   then n_records lines  flags barcode_as_hex name_as_hex secondary umi_as_hex     ("-" for an empty string)
// For both cell rules -- the streamed one (ParseCellsStream) and the any-order one (collate_barcodes_host on the
// survivors) -- and both name modes, the survivors are laid out by cell as the arena is, and for EVERY partition of the
// cells into consecutive groups dedup_umis_host runs per group on arrays of exactly the group's size, dedup_drop_host
// drops its duplicates and the pieces are joined as barcodes_stream_assemble joins them.  Prints per rule and mode
//   ok <rule> <mode> <partitions> | order' (as stream indices) | group_off' | cell_group_off' | cell_rec_off' | cell_dups
// or  differs <what> <partition as a bit mask>.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "oarfish_em.h"

#include "../../oarfish_amd/csrc/oem_collate.h"

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
static std::string unhex(const char *hex)
{
    std::string s;
    if (hex[0] != '-')
        for (size_t k = 0; hex[k] && hex[k + 1]; k += 2) s.push_back((char)(hexval(hex[k]) * 16 + hexval(hex[k + 1])));
    return s;
}

struct Blob { // strings as the ABI takes them, at their exact sizes
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off{0};
    void add(const std::string &s)
    {
        bytes.insert(bytes.end(), s.begin(), s.end());
        off.push_back(bytes.size());
    }
};

struct Walk {
    std::vector<uint64_t> order, group_off, cell_group_off, cell_rec_off, cell_dups;
    bool operator==(const Walk &o) const
    {
        return order == o.order && group_off == o.group_off && cell_group_off == o.cell_group_off && cell_rec_off == o.cell_rec_off &&
               cell_dups == o.cell_dups;
    }
};

// The cells [c0, c1) of a layout by cell (names, flags, UMIs per laid-out survivor; cro: the cells' first survivors):
// collated, deduplicated and dropped on group-local indices; the UMIs' offsets are the layout's, seen through the
// group's window, and their bytes stay where they are.
static void run_group(const Blob &names, const std::vector<uint8_t> &sec, const Blob &umis, const std::vector<uint64_t> &cro, uint32_t c0,
                      uint32_t c1, uint32_t mode, Walk *out, uint64_t *pos_base, uint64_t *group_base)
{
    const uint64_t r0 = cro[c0], m = cro[c1] - r0;
    const uint32_t nc = c1 - c0;
    std::vector<uint8_t> gnames(names.bytes.begin() + names.off[r0], names.bytes.begin() + names.off[r0 + m]), gsec(sec.begin() + r0, sec.begin() + r0 + m);
    std::vector<uint64_t> goff_names(m + 1), gcro(nc + 1);
    for (uint64_t i = 0; i <= m; ++i) goff_names[i] = names.off[r0 + i] - names.off[r0];
    for (uint32_t c = 0; c <= nc; ++c) gcro[c] = cro[c0 + c] - r0;
    std::vector<uint32_t> order(m);
    std::vector<uint64_t> goff(m + 1), cgo(nc + 1);
    uint64_t ng = 0;
    bool zero = false;
    if (oem::collate_host(gnames.data(), goff_names.data(), gsec.data(), m, gcro.data(), nc, mode, order.data(), goff.data(), &ng, cgo.data(),
                          &zero) != oem::kCollateNoRecord)
        exit(4);
    goff.resize(ng + 1);
    std::vector<uint64_t> window(umis.off.begin() + r0, umis.off.begin() + r0 + m + 1); // exactly the group's m + 1 offsets
    std::vector<uint8_t> dup(ng);
    std::vector<uint64_t> survivor(ng), cell_dups(nc);
    oem::dedup_umis_host(umis.bytes.data(), window.data(), nullptr, order.data(), goff.data(), ng, cgo.data(), nc, dup.data(), survivor.data(),
                         cell_dups.data());
    uint64_t n_dups = 0, removed = 0;
    for (uint64_t g = 0; g < ng; ++g)
        if (dup[g]) {
            ++n_dups;
            removed += goff[g + 1] - goff[g];
        }
    std::vector<uint32_t> order2(m - removed);
    std::vector<uint64_t> goff2(ng - n_dups + 1), cgo2(nc + 1), cro2(nc + 1);
    if (oem::dedup_drop_host(order.data(), goff.data(), ng, cgo.data(), nc, dup.data(), order2.data(), goff2.data(), cgo2.data(), cro2.data()) !=
        ng - n_dups)
        exit(3);
    // the join: every later group's place depends on what the earlier ones lost
    for (uint32_t v : order2) out->order.push_back(r0 + v);
    for (uint64_t g = 0; g < ng - n_dups; ++g) out->group_off.push_back(*pos_base + goff2[g]);
    for (uint32_t c = 1; c <= nc; ++c) {
        out->cell_group_off.push_back(*group_base + cgo2[c]);
        out->cell_rec_off.push_back(*pos_base + cro2[c]);
    }
    out->cell_dups.insert(out->cell_dups.end(), cell_dups.begin(), cell_dups.end());
    *pos_base += order2.size();
    *group_base += ng - n_dups;
}

static void put(const std::vector<uint64_t> &v)
{
    printf(" |");
    for (uint64_t x : v) printf(" %" PRIu64, x);
}

int main()
{
    uint64_t n;
    if (scanf("%" SCNu64, &n) != 1 || n < 1 || n > 20) return 2;
    std::vector<oem_aln_record> rec(n);
    std::vector<std::string> bc(n), nm(n), um(n);
    std::vector<uint8_t> sec(n);
    Blob all_bc;
    for (uint64_t i = 0; i < n; ++i) {
        char h1[256], h2[256], h3[256];
        uint32_t flags, s;
        if (scanf("%" SCNu32 " %255s %255s %" SCNu32 " %255s", &flags, h1, h2, &s, h3) != 5) return 2;
        memset(&rec[i], 0, sizeof rec[i]);
        rec[i].flags = flags;
        bc[i] = unhex(h1), nm[i] = unhex(h2), um[i] = unhex(h3);
        sec[i] = (uint8_t)s;
        all_bc.add(bc[i]);
    }
    // S and the streamed cells
    oem::ParseCellsStream st;
    st.push(rec.data(), n, all_bc.bytes.data(), all_bc.off.data());
    st.finish();
    const std::vector<uint64_t> &S = st.survivors;
    const uint64_t ns = S.size();
    if (!ns) return 2;
    for (int rule = 0; rule < 2; ++rule) {
        // the layout by cell: lay[k] = the survivor (a position of S) at arena position k, and the cells' first positions
        std::vector<uint32_t> lay(ns);
        std::vector<uint64_t> cro;
        if (rule == 0) {
            for (uint64_t k = 0; k < ns; ++k) lay[k] = (uint32_t)k;
            cro = st.cell_rec_off;
        } else {
            Blob sbc;
            for (uint64_t k = 0; k < ns; ++k) sbc.add(bc[S[k]]);
            cro.assign(ns + 1, 0);
            uint64_t nc = 0;
            bool zero = false;
            if (oem::collate_barcodes_host(sbc.bytes.data(), sbc.off.data(), ns, lay.data(), cro.data(), &nc, &zero) != oem::kCollateNoRecord) return 4;
            cro.resize(nc + 1);
        }
        const uint32_t nc = (uint32_t)(cro.size() - 1);
        if (nc < 1 || nc > 12) return 2;
        Blob names, umis;
        std::vector<uint8_t> lsec(ns);
        for (uint64_t k = 0; k < ns; ++k) {
            names.add(nm[S[lay[k]]]);
            umis.add(um[S[lay[k]]]);
            lsec[k] = sec[S[lay[k]]];
        }
        if (oem::dedup_first_bad_umi(umis.bytes.data(), umis.off.data(), ns) != oem::kCollateNoRecord) return 5;
        for (uint32_t mode : {oem::kCollateSort, oem::kCollateAdjacent}) {
            auto run = [&](uint64_t mask) { // bit c - 1 set: a group starts at cell c
                Walk w;
                w.cell_group_off.push_back(0);
                w.cell_rec_off.push_back(0);
                uint64_t pos_base = 0, group_base = 0;
                uint32_t c0 = 0;
                for (uint32_t c = 1; c <= nc; ++c)
                    if (c == nc || (mask >> (c - 1) & 1)) {
                        run_group(names, lsec, umis, cro, c0, c, mode, &w, &pos_base, &group_base);
                        c0 = c;
                    }
                w.group_off.push_back(pos_base);
                return w;
            };
            const Walk whole = run(0);
            uint64_t partitions = 0;
            for (uint64_t mask = 0; mask < (1ull << (nc - 1)); ++mask, ++partitions)
                if (!(run(mask) == whole)) {
                    printf("differs %s %" PRIu64 "\n", rule ? "any-order" : "streamed", mask);
                    return 1;
                }
            printf("ok %s %s %" PRIu64, rule ? "any-order" : "streamed", mode == oem::kCollateSort ? "sort" : "adjacent", partitions);
            std::vector<uint64_t> order64;
            for (uint64_t v : whole.order) order64.push_back(S[lay[v]]);
            put(order64);
            put(whole.group_off);
            put(whole.cell_group_off);
            put(whole.cell_rec_off);
            put(whole.cell_dups);
            putchar('\n');
        }
    }
    return 0;
}
