// oem_collate.h -- collating a cell's alignment records by read name, as pure host / device functions.
//
// Reference (COMBINE-lab/oarfish v0.10.3, src/alignment_parser.rs): in single-cell mode the input is collated by barcode
// only, so sort_and_parse_barcode_records (:170-241) first sorts the cell's records by read name with a read's primary
// record before its secondaries (:180-191) and then cuts a group wherever the name changes (:201-239).  The bulk parser
// (:301-437) takes name-collated input and only cuts.  Both are stated here once; the kernels of oem_collate_device.hip,
// the host walk below (the testing library's oem_test_collate_host, the stand-alone program of tests/test_collate.py)
// and the documentation of oem_collate_names all refer to this file.
//
// The order inside a cell, for records i and j:
//   1. the names as bytes, unsigned and lexicographic, a proper prefix first (<[u8]>::cmp, what x.name().cmp(&y.name())
//      does);
//   2. secondary != 0 after secondary == 0 (the primary first);
//   3. the record index.
// The reference's sort is unstable and its comparator calls two secondaries of one read (and two primaries, "this one
// shouldn't happen") equal, so it leaves their order open.  Rule 3 is the stable choice: one of the orders the
// reference's comparator allows, and the one every implementation here gives.
//
// A group is a maximal run of identical names inside one cell: the same name in two cells gives two groups.  In
// kCollateAdjacent mode nothing is sorted; a group ends where the name differs from the previous record's or where a
// cell ends.
//
// Names are never empty (the reference skips such records at :202, the hook drops them before calling) and hold no 0
// byte (a BAM read name cannot).  The second condition lets a name be compared through zero-padded keys: key r of a name
// is its bytes [8r, 8r + 8) as one big-endian u64, zero past the end.  Comparing names equals comparing their key
// sequences; two names whose keys agree up to and including a key whose last byte is 0 are the same name.
//
// Cells from barcodes (collate_barcodes_host below, oem_collate_barcodes): the reference takes input whose records are
// adjacent per barcode (single_cell.rs:196-213 reads the CB tag of a run's first record, alignment_parser.rs:244-299
// cuts where it changes; docs/index.md "all records of a barcode must be adjacent").  Here the records may come in any
// order:
//   - a cell is the set of records with one barcode, the barcodes compared as bytes;
//   - cells are numbered in the order of their first record in the input (first seen), so input that is collated by
//     barcode already gives the cells it gives today, in the same order;
//   - inside a cell the records keep their input order (the name rule above is applied afterwards, inside each cell);
//   - order_bc is the cell-major permutation of the records, cell_rec_off[c] cell c's first position in it, n_cells the
//     number of distinct barcodes.
// A barcode is never empty (the reference bails when CB is missing: single_cell.rs:203, alignment_parser.rs:150) and
// holds no 0 byte: the conditions names carry, and what lets the same zero-padded keys sort them.
//
// The bulk parser (parse_bulk_host below, oem_store_create_records_names): alignment_parser.rs:301-437, parse_alignments,
// from records and read names in input order to the groups AlignmentFilters::filter takes.
//   skip     a record with OEM_REC_UNMAPPED takes no part in anything below (:367-370): it cuts no read, its name is
//            never looked at (it may be empty or hold a 0 byte), and a read made only of such records is no group at
//            all, so it is no `no_mapping` entry of the discard table either.  n_unmapped counts these records,
//            n_parsed = n_records - n_unmapped.  (The reference also drops a mapped record that has no reference id,
//            :377 and :410; oem_aln_record has no such state -- every record that is not unmapped carries a ref_id --
//            so there is nothing to build for it.)
//   names    the names of the surviving records are not empty and hold no 0 byte; the first violation, by the record's
//            index in the caller's input, is an error.
//   order    kCollateAdjacent is the reference's parser: `order` is the surviving input indices, ascending, and a group
//            is a maximal run of identical names in it -- `A, unmapped, A` is one group of two whatever the unmapped
//            record is called.  kCollateSort lifts the requirement that the input be name-collated: `order` is the
//            surviving indices sorted by the name rule above (name bytes, primary before secondary, index), all of
//            them as one cell, and the groups are cut the same way.
//   check    under kCollateAdjacent with sort_check_num = N > 0 the first min(N, n_groups) groups are checked (:396-408,
//            prog_opts.rs:558-561, N = 100 000 there): if the name of a checked group g equals the name of an earlier
//            group the input is not name-collated and the call fails, naming the smallest such g, the input index of
//            its first record and that of the earlier group's first record.  A repeat at a group index >= N is not an
//            error (the reference's behaviour), N = 0 is no check, and under kCollateSort there is nothing to check.
//   filter   oem_filter.h unchanged over the groups in order; row r of the store is the r-th group with kept > 0, its
//            name the name of the first record of its group (the name_vec of :341-351), and unique_alignments is the
//            number of groups with kept == 1 (:386-388: after add_group returned true records_for_read holds what
//            filter retained, oarfish_types.rs:987, :1121).
#pragma once

#include <stdint.h>
#include <string.h>

#ifndef OEM_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define OEM_HD __host__ __device__
#else
#define OEM_HD
#endif
#endif

#include <algorithm>
#include <vector>

#include "oem_barcode_table.h"

namespace oem {

enum : uint32_t { kCollateSort = 0, kCollateAdjacent = 1 };
constexpr uint64_t kCollateNoRecord = ~0ull;

// key `round` of the name at p[0 .. len)
OEM_HD inline uint64_t collate_key(const uint8_t *p, uint64_t len, uint64_t round)
{
    uint64_t k = 0;
    for (uint64_t b = 0; b < 8; ++b) {
        const uint64_t at = 8 * round + b;
        k = (k << 8) | (at < len ? (uint64_t)p[at] : 0ull);
    }
    return k;
}

// a name's keys are over once one of them ends in a 0 byte
OEM_HD inline bool collate_key_is_last(uint64_t key) { return (key & 0xffull) == 0; }

// <[u8]>::cmp
OEM_HD inline int collate_name_cmp(const uint8_t *a, uint64_t la, const uint8_t *b, uint64_t lb)
{
    const uint64_t n = la < lb ? la : lb;
    for (uint64_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

// the whole key of the order: is record i before record j?
inline bool collate_before(const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary, uint32_t i, uint32_t j)
{
    const int c = collate_name_cmp(names + name_off[i], name_off[i + 1] - name_off[i], names + name_off[j], name_off[j + 1] - name_off[j]);
    if (c) return c < 0;
    const bool si = secondary && secondary[i], sj = secondary && secondary[j];
    if (si != sj) return sj;
    return i < j;
}

// The first record (kCollateNoRecord: none) with an empty name, or with a 0 byte in its name; *zero_byte tells which.
inline uint64_t collate_first_bad_name(const uint8_t *names, const uint64_t *name_off, uint64_t n_records, bool *zero_byte)
{
    for (uint64_t i = 0; i < n_records; ++i) {
        const uint64_t len = name_off[i + 1] - name_off[i];
        const bool z = len && memchr(names + name_off[i], 0, len);
        if (!len || z) {
            *zero_byte = z;
            return i;
        }
    }
    return kCollateNoRecord;
}

// One cell of the host walk: order[r0 .. r1) sorted (or the identity), the group starts appended to group_off.
inline void collate_host_cell(const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary, uint64_t r0, uint64_t r1,
                              uint32_t mode, uint32_t *order)
{
    for (uint64_t i = r0; i < r1; ++i) order[i] = (uint32_t)i;
    if (mode == kCollateSort)
        std::sort(order + r0, order + r1, [&](uint32_t i, uint32_t j) { return collate_before(names, name_off, secondary, i, j); });
}

// The cut: the positions of `order` where a read starts, cell by cell, then n_records; cell_group_off from them.
inline void collate_host_cut(const uint8_t *names, const uint64_t *name_off, uint64_t n_records, const uint64_t *cell_rec_off,
                             uint32_t n_cells, const uint32_t *order, uint64_t *group_off, uint64_t *n_groups, uint64_t *cell_group_off)
{
    uint64_t g = 0;
    for (uint32_t c = 0; c < n_cells; ++c) {
        cell_group_off[c] = g;
        for (uint64_t p = cell_rec_off[c]; p < cell_rec_off[c + 1]; ++p) {
            bool head = p == cell_rec_off[c];
            if (!head) {
                const uint32_t i = order[p], j = order[p - 1];
                head = collate_name_cmp(names + name_off[i], name_off[i + 1] - name_off[i], names + name_off[j], name_off[j + 1] - name_off[j]) != 0;
            }
            if (head) group_off[g++] = p;
        }
    }
    cell_group_off[n_cells] = g;
    group_off[g] = n_records;
    *n_groups = g;
}

// The host walk of the whole rule (arguments as oem_collate_names, already checked).  Returns the first bad record as
// collate_first_bad_name does, and then leaves the outputs alone.
inline uint64_t collate_host(const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary, uint64_t n_records,
                             const uint64_t *cell_rec_off, uint32_t n_cells, uint32_t mode, uint32_t *order, uint64_t *group_off,
                             uint64_t *n_groups, uint64_t *cell_group_off, bool *zero_byte)
{
    const uint64_t bad = collate_first_bad_name(names, name_off, n_records, zero_byte);
    if (bad != kCollateNoRecord) return bad;
    for (uint32_t c = 0; c < n_cells; ++c) collate_host_cell(names, name_off, secondary, cell_rec_off[c], cell_rec_off[c + 1], mode, order);
    collate_host_cut(names, name_off, n_records, cell_rec_off, n_cells, order, group_off, n_groups, cell_group_off);
    return kCollateNoRecord;
}

// The host walk of the barcode rule: a stable sort of the records by barcode bytes, the runs of one barcode ranked by
// their first (= smallest, the sort being stable) record, and the runs laid out in that rank.  order (n_records),
// cell_rec_off (capacity n_records + 1; *n_cells + 1 written).  Returns the first bad barcode as collate_first_bad_name
// does, and then leaves the outputs alone.
inline uint64_t collate_barcodes_host(const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n_records, uint32_t *order,
                                      uint64_t *cell_rec_off, uint64_t *n_cells, bool *zero_byte)
{
    const uint64_t bad = collate_first_bad_name(barcodes, barcode_off, n_records, zero_byte);
    if (bad != kCollateNoRecord) return bad;
    auto cmp = [&](uint32_t i, uint32_t j) {
        return collate_name_cmp(barcodes + barcode_off[i], barcode_off[i + 1] - barcode_off[i], barcodes + barcode_off[j],
                                barcode_off[j + 1] - barcode_off[j]);
    };
    std::vector<uint32_t> sorted(n_records);
    for (uint64_t i = 0; i < n_records; ++i) sorted[i] = (uint32_t)i;
    std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t i, uint32_t j) { return cmp(i, j) < 0; });
    std::vector<uint64_t> run_off; // the positions of `sorted` where a barcode starts, then n_records
    for (uint64_t p = 0; p < n_records; ++p)
        if (p == 0 || cmp(sorted[p - 1], sorted[p]) != 0) run_off.push_back(p);
    const uint64_t n_runs = run_off.size();
    run_off.push_back(n_records);
    std::vector<uint64_t> by_head(n_runs);
    for (uint64_t r = 0; r < n_runs; ++r) by_head[r] = r;
    std::sort(by_head.begin(), by_head.end(), [&](uint64_t a, uint64_t b) { return sorted[run_off[a]] < sorted[run_off[b]]; });
    uint64_t at = 0;
    for (uint64_t c = 0; c < n_runs; ++c) {
        cell_rec_off[c] = at;
        for (uint64_t p = run_off[by_head[c]]; p < run_off[by_head[c] + 1]; ++p) order[at++] = sorted[p];
    }
    cell_rec_off[n_runs] = n_records;
    *n_cells = n_runs;
    return kCollateNoRecord;
}

constexpr uint32_t kRecUnmapped = 1u; // OEM_REC_UNMAPPED

// UMI deduplication (dedup_umis_host below, oem_dedup_umis, oem_em_run_cells_records_umis_sparse).  Nothing of this is in
// the reference: its documentation (docs/index.md:308-312) wants single-cell input "with already (UMI) deduplicated
// reads" -- "a count will be obtained for each read record" -- and names UMI counting as future work.  This rule lifts
// that requirement for input whose UB tags are corrected already.
// Input: a collated order as the barcode and name rules above leave it -- order (position k holds a caller input index),
// group_off (n_groups + 1; a group is a read), cell_group_off (n_cells + 1) -- one UMI byte string per INPUT record (a
// record without a UB tag has the empty string; a UMI holds no 0 byte, which is the caller's to check:
// dedup_first_bad_umi) and the records' flags.
//   head(g)   order[group_off[g]], the read's first record in collated order: under kCollateSort its primary.
//   umi(g)    the UMI of record head(g).  The UMIs of a read's other records are not examined.
//   takes part   group g takes part iff it has a record, umi(g) is not empty and record head(g) does not have
//             OEM_REC_UNMAPPED.  A group that does not take part is never a duplicate and never shadows another: an
//             unmapped read cannot hide a mapped read of the same molecule.
//   class     inside one cell, the groups that take part and whose UMIs are byte-identical (same length, same bytes:
//             ACG and ACGT differ).  Classes never span cells.
//   survivor  of a class: its smallest group index.  Every other member is a duplicate.  Under kCollateSort the groups
//             of a cell are in name order, so the survivor is the read whose name sorts first and the result does not
//             depend on the input's order; under kCollateAdjacent it is the first read in input order.
//   results   dup[g] (0 / 1); survivor[g], the survivor's group index for a duplicate and g itself otherwise;
//             cell_dups[c], the duplicates of cell c; and the DEDUPLICATED COLLATION order', group_off', cell_group_off',
//             cell_rec_off': the same arrays with the duplicate groups' positions removed and everything else in place
//             (dedup_drop_host).  No cell becomes empty through this: every class keeps one member.
//
// The UMI rule (dedup_umis_rule_host below, oem_dedup_umis_rule, oem_em_run_cells_records_umis_rule_sparse) is
// (gene_of, correct): gene_of is NULL or one uint32 gene id per transcript, correct is 0 or 1.  With gene_of == NULL and
// correct == 0 everything below reduces to the rule above, result for result.  head, "takes part" and the cell
// boundaries stay as they are.
//   gene(g)   gene_of[ref_id(head(g))]: the gene of the read's first record in collated order, under kCollateSort its
//             primary's.  0 for every group when gene_of is NULL.  Only groups that take part are looked up (their head
//             is mapped, so it has a ref_id); a ref_id that is not below n_txps is an error naming the smallest such
//             input index.
//   segment   the groups of one cell that take part and share gene(g).  A class is now the set of groups of one segment
//             with byte-identical UMIs; n(u) is the number of groups in class u.
//   neighbour two classes u != v of one segment are neighbours iff their UMIs have the same length and differ in exactly
//             one byte position.  Any bytes: there is no alphabet (N, lower case and 0xff are bytes like any other).
//   parent    (only with correct) parent(u) is chosen among the neighbours v with n(v) > n(u) -- strictly, so there are
//             no cycles: the one with the greatest n(v), among equals the one whose UMI bytes compare smallest
//             (collate_name_cmp).  No such neighbour: no parent.  Parents are chosen from the ORIGINAL counts.
//   root      root(u) follows parent until a class has none; the counts rise strictly along the way.
//   molecule  the groups of all classes with one root.  Its survivor is its smallest group index, every other member is
//             a duplicate of it: the convention above, so under kCollateSort the result still does not depend on the
//             input's order.
//   corrected a group whose class has a parent; cell_corrected[c] counts them.  A corrected group may itself be its
//             molecule's survivor.
//   results   dup, survivor, cell_dups as above, and cell_corrected.  No cell becomes empty; groups that do not take
//             part are untouched and shadow nothing.
// Limits, on purpose: the gene of a read that maps to several genes is its head's; one mismatch only, no indels (this is
// Cell Ranger's rule, not umi_tools' directional network); the survivor is not chosen by read length or by what the
// filter keeps -- deduplication still runs before the filter.  Without a rule (dedup_umis_host, the sessions) matching
// is exact, on corrected UMIs (umi_tools' `unique` method), and the key is (cell, UMI), with no gene in it.

// The first input record (kCollateNoRecord: none) whose UMI holds a 0 byte.  Empty UMIs are legal.
inline uint64_t dedup_first_bad_umi(const uint8_t *umis, const uint64_t *umi_off, uint64_t n_records)
{
    for (uint64_t i = 0; i < n_records; ++i) {
        const uint64_t len = umi_off[i + 1] - umi_off[i];
        if (len && memchr(umis + umi_off[i], 0, len)) return i;
    }
    return kCollateNoRecord;
}

// The host walk of the UMI rule: the specification.  flags: one word per input record, or NULL (none unmapped).  dup
// (n_groups), survivor (n_groups), cell_dups (n_cells).  The arguments are checked by the caller.
inline void dedup_umis_host(const uint8_t *umis, const uint64_t *umi_off, const uint32_t *flags, const uint32_t *order,
                            const uint64_t *group_off, uint64_t n_groups, const uint64_t *cell_group_off, uint32_t n_cells, uint8_t *dup,
                            uint64_t *survivor, uint64_t *cell_dups)
{
    for (uint64_t g = 0; g < n_groups; ++g) {
        dup[g] = 0;
        survivor[g] = g;
    }
    auto head = [&](uint64_t g) { return order[group_off[g]]; };
    auto cmp = [&](uint64_t a, uint64_t b) {
        const uint32_t i = head(a), j = head(b);
        return collate_name_cmp(umis + umi_off[i], umi_off[i + 1] - umi_off[i], umis + umi_off[j], umi_off[j + 1] - umi_off[j]);
    };
    std::vector<uint64_t> part;
    for (uint32_t c = 0; c < n_cells; ++c) {
        cell_dups[c] = 0;
        part.clear();
        for (uint64_t g = cell_group_off[c]; g < cell_group_off[c + 1]; ++g) {
            if (group_off[g + 1] == group_off[g]) continue;
            const uint32_t i = head(g);
            if (umi_off[i + 1] > umi_off[i] && !(flags && (flags[i] & kRecUnmapped))) part.push_back(g);
        }
        std::sort(part.begin(), part.end(), [&](uint64_t a, uint64_t b) {
            const int r = cmp(a, b);
            return r ? r < 0 : a < b;
        });
        for (size_t k = 1, first = 0; k < part.size(); ++k) { // a run's first member is its smallest group: the survivor
            if (cmp(part[first], part[k]) != 0) {
                first = k;
                continue;
            }
            dup[part[k]] = 1;
            survivor[part[k]] = part[first];
            ++cell_dups[c];
        }
    }
}

// Two UMIs of one length that differ in exactly one byte position.
OEM_HD inline bool dedup_umis_neighbours(const uint8_t *a, uint64_t la, const uint8_t *b, uint64_t lb)
{
    if (la != lb) return false;
    uint64_t differ = 0;
    for (uint64_t i = 0; i < la; ++i) differ += a[i] != b[i] ? 1 : 0;
    return differ == 1;
}

// The host walk of the UMI rule (gene_of, correct): the specification, all pairs inside a segment.  ref_id: one word per
// input record, read only with gene_of and only at the heads of groups that take part; cell_corrected (n_cells) may be
// NULL.  Returns kCollateNoRecord, or the smallest input index of such a head whose ref_id is not below n_txps, and
// then leaves the outputs alone.  The other arguments are dedup_umis_host's, checked by the caller.
inline uint64_t dedup_umis_rule_host(const uint8_t *umis, const uint64_t *umi_off, const uint32_t *flags, const uint32_t *ref_id,
                                     const uint32_t *gene_of, uint32_t n_txps, uint32_t correct, const uint32_t *order,
                                     const uint64_t *group_off, uint64_t n_groups, const uint64_t *cell_group_off, uint32_t n_cells,
                                     uint8_t *dup, uint64_t *survivor, uint64_t *cell_dups, uint64_t *cell_corrected)
{
    auto head = [&](uint64_t g) { return order[group_off[g]]; };
    auto takes_part = [&](uint64_t g) {
        if (group_off[g + 1] == group_off[g]) return false;
        const uint32_t i = head(g);
        return umi_off[i + 1] > umi_off[i] && !(flags && (flags[i] & kRecUnmapped));
    };
    if (gene_of) {
        uint64_t bad = kCollateNoRecord;
        for (uint64_t g = 0; g < n_groups; ++g)
            if (takes_part(g) && ref_id[head(g)] >= n_txps) bad = std::min<uint64_t>(bad, head(g));
        if (bad != kCollateNoRecord) return bad;
    }
    for (uint64_t g = 0; g < n_groups; ++g) {
        dup[g] = 0;
        survivor[g] = g;
    }
    auto gene = [&](uint64_t g) { return gene_of ? gene_of[ref_id[head(g)]] : 0u; };
    auto umi = [&](uint64_t g) { return umis + umi_off[head(g)]; };
    auto len = [&](uint64_t g) { return umi_off[(uint64_t)head(g) + 1] - umi_off[head(g)]; };
    auto cmp = [&](uint64_t a, uint64_t b) { return collate_name_cmp(umi(a), len(a), umi(b), len(b)); };
    std::vector<uint64_t> part, first, parent; // first: where a class starts in part, then part.size()
    for (uint32_t c = 0; c < n_cells; ++c) {
        cell_dups[c] = 0;
        if (cell_corrected) cell_corrected[c] = 0;
        part.clear();
        for (uint64_t g = cell_group_off[c]; g < cell_group_off[c + 1]; ++g)
            if (takes_part(g)) part.push_back(g);
        std::sort(part.begin(), part.end(), [&](uint64_t a, uint64_t b) {
            if (gene(a) != gene(b)) return gene(a) < gene(b);
            const int r = cmp(a, b);
            return r ? r < 0 : a < b;
        });
        first.clear();
        for (size_t k = 0; k < part.size(); ++k)
            if (k == 0 || gene(part[k - 1]) != gene(part[k]) || cmp(part[k - 1], part[k]) != 0) first.push_back(k);
        const size_t n_classes = first.size();
        first.push_back(part.size());
        auto rep = [&](size_t u) { return part[first[u]]; }; // a class's smallest group
        auto count = [&](size_t u) { return first[u + 1] - first[u]; };
        parent.assign(n_classes, kCollateNoRecord);
        for (size_t s0 = 0, s1 = 0; correct && s0 < n_classes; s0 = s1) { // a segment: the classes [s0, s1) of one gene
            for (s1 = s0 + 1; s1 < n_classes && gene(rep(s1)) == gene(rep(s0));) ++s1;
            for (size_t u = s0; u < s1; ++u)
                for (size_t v = s0; v < s1; ++v) {
                    if (v == u || count(v) <= count(u)) continue;
                    if (!dedup_umis_neighbours(umi(rep(u)), len(rep(u)), umi(rep(v)), len(rep(v)))) continue;
                    const uint64_t p = parent[u];
                    if (p == kCollateNoRecord || count(v) > count(p) || (count(v) == count(p) && cmp(rep(v), rep(p)) < 0)) parent[u] = v;
                }
        }
        std::vector<uint64_t> root(n_classes), least(n_classes, kCollateNoRecord); // least: a root's molecule's smallest group
        for (size_t u = 0; u < n_classes; ++u) {
            size_t r = u;
            while (parent[r] != kCollateNoRecord) r = parent[r];
            root[u] = r;
            least[r] = std::min(least[r], rep(u));
        }
        for (size_t u = 0; u < n_classes; ++u)
            for (uint64_t k = first[u]; k < first[u + 1]; ++k) {
                const uint64_t g = part[k];
                if (parent[u] != kCollateNoRecord && cell_corrected) ++cell_corrected[c];
                if (g == least[root[u]]) continue;
                dup[g] = 1;
                survivor[g] = least[root[u]];
                ++cell_dups[c];
            }
    }
    return kCollateNoRecord;
}

// The deduplicated collation: the positions of the duplicate groups removed.  out_order (capacity n_positions),
// out_group_off (capacity n_groups + 1), out_cell_group_off and out_cell_rec_off (n_cells + 1 each).  Returns the number
// of groups that remain.
inline uint64_t dedup_drop_host(const uint32_t *order, const uint64_t *group_off, uint64_t n_groups, const uint64_t *cell_group_off,
                                uint32_t n_cells, const uint8_t *dup, uint32_t *out_order, uint64_t *out_group_off,
                                uint64_t *out_cell_group_off, uint64_t *out_cell_rec_off)
{
    uint64_t at = 0, ng = 0;
    for (uint32_t c = 0; c < n_cells; ++c) {
        out_cell_group_off[c] = ng;
        out_cell_rec_off[c] = at;
        for (uint64_t g = cell_group_off[c]; g < cell_group_off[c + 1]; ++g) {
            if (dup[g]) continue;
            out_group_off[ng++] = at;
            for (uint64_t p = group_off[g]; p < group_off[g + 1]; ++p) out_order[at++] = order[p];
        }
    }
    out_cell_group_off[n_cells] = ng;
    out_cell_rec_off[n_cells] = at;
    out_group_off[ng] = at;
    return ng;
}

// What the host walk of the bulk parser finds besides order and group_off.
struct ParseBulk {
    uint64_t n_unmapped = 0, n_parsed = 0, n_groups = 0, n_checked = 0;
    uint64_t bad_record = kCollateNoRecord;   // the first surviving record with a bad name (input index); zero_byte tells which
    bool zero_byte = false;
    uint64_t repeat_group = kCollateNoRecord; // the collation check: the smallest checked group whose name an earlier group has,
    uint64_t repeat_record = 0, earlier_record = 0; // the input indices of its first record and of the earlier group's
};

// The host walk of the bulk rule.  Rec: any record with a `flags` word (oem_aln_record).  order (capacity n_records;
// n_parsed written), group_off (capacity n_records + 1; n_groups + 1 written).  With a bad name nothing but the counts
// and bad_record is filled; with a repeat everything is.
template <typename Rec>
inline ParseBulk parse_bulk_host(const Rec *records, uint64_t n_records, const uint8_t *names, const uint64_t *name_off,
                                 const uint8_t *secondary, uint32_t mode, uint64_t sort_check_num, uint32_t *order, uint64_t *group_off)
{
    ParseBulk pb;
    uint64_t m = 0;
    for (uint64_t i = 0; i < n_records; ++i) {
        if (records[i].flags & kRecUnmapped) continue;
        const uint64_t len = name_off[i + 1] - name_off[i];
        const bool z = len && memchr(names + name_off[i], 0, len);
        if ((!len || z) && pb.bad_record == kCollateNoRecord) {
            pb.bad_record = i;
            pb.zero_byte = z;
        }
        order[m++] = (uint32_t)i;
    }
    pb.n_parsed = m;
    pb.n_unmapped = n_records - m;
    if (pb.bad_record != kCollateNoRecord) return pb;
    if (mode == kCollateSort)
        std::sort(order, order + m, [&](uint32_t i, uint32_t j) { return collate_before(names, name_off, secondary, i, j); });
    auto same = [&](uint32_t i, uint32_t j) {
        return collate_name_cmp(names + name_off[i], name_off[i + 1] - name_off[i], names + name_off[j], name_off[j + 1] - name_off[j]) == 0;
    };
    uint64_t g = 0;
    for (uint64_t p = 0; p < m; ++p)
        if (p == 0 || !same(order[p], order[p - 1])) group_off[g++] = p;
    group_off[g] = m;
    pb.n_groups = g;
    if (mode == kCollateAdjacent && sort_check_num) {
        const uint64_t nc = sort_check_num < g ? sort_check_num : g;
        pb.n_checked = nc;
        std::vector<uint64_t> by_name(nc); // the checked groups sorted by the name of their head, then by group index
        for (uint64_t k = 0; k < nc; ++k) by_name[k] = k;
        auto head = [&](uint64_t k) { return order[group_off[k]]; };
        std::sort(by_name.begin(), by_name.end(), [&](uint64_t a, uint64_t b) {
            const uint32_t i = head(a), j = head(b);
            const int c = collate_name_cmp(names + name_off[i], name_off[i + 1] - name_off[i], names + name_off[j], name_off[j + 1] - name_off[j]);
            return c ? c < 0 : a < b;
        });
        for (uint64_t k = 1; k < nc; ++k) { // a run's second member is the first group to repeat the run's name
            if (!same(head(by_name[k]), head(by_name[k - 1]))) continue;
            if (k >= 2 && same(head(by_name[k - 1]), head(by_name[k - 2]))) continue;
            if (by_name[k] < pb.repeat_group) {
                pb.repeat_group = by_name[k];
                pb.repeat_record = head(by_name[k]);
                pb.earlier_record = head(by_name[k - 1]);
            }
        }
    }
    return pb;
}

// The streamed form of parse_bulk_host, for kCollateAdjacent only: the same input cut into batches at ANY record
// positions (oem_records_stream_push_names), a cut inside a read included.  This is the one statement of how a batch's
// surviving records attach to the open read:
//   - a batch's survivors are its records without OEM_REC_UNMAPPED, in input order;
//   - the open read (the carry) is the trailing run of one name among all survivors pushed so far;
//   - a batch's first run joins the carry when its name is the carry's name, byte for byte; otherwise the carry is
//     closed before the batch's first run;
//   - every run of the batch but the last is closed by the batch itself, the last run becomes the new carry;
//   - a batch without a survivor (an empty batch, a batch of unmapped records only) changes nothing but the counts;
//   - finish closes the carry.
// Groups are numbered in closing order.  A group's head is its first record's session-global input index: 64-bit, it
// counts all records of all pushed batches in push order, unmapped ones included.  The names of surviving records are
// the caller's to check (collate_first_bad_name's conditions); unmapped records' names are never read.
struct ParseBulkStream {
    uint64_t n_records = 0, n_unmapped = 0;       // of all batches pushed
    std::vector<uint64_t> group_size, group_head; // the closed groups
    bool open = false;                            // the carry: its name, its size so far and its head
    std::vector<uint8_t> open_name;
    uint64_t open_size = 0, open_head = 0;

    void close()
    {
        if (!open) return;
        group_size.push_back(open_size);
        group_head.push_back(open_head);
        open = false;
        open_size = 0;
    }
    template <typename Rec>
    void push(const Rec *records, uint64_t n, const uint8_t *names, const uint64_t *name_off)
    {
        for (uint64_t i = 0; i < n; ++i) {
            if (records[i].flags & kRecUnmapped) {
                ++n_unmapped;
                continue;
            }
            const uint8_t *nm = names + name_off[i];
            const uint64_t len = name_off[i + 1] - name_off[i];
            if (!open || collate_name_cmp(nm, len, open_name.data(), open_name.size()) != 0) {
                close();
                open = true;
                open_name.assign(nm, nm + len);
                open_head = n_records + i;
            }
            ++open_size;
        }
        n_records += n;
    }
    void finish() { close(); }
};

// The streamed form of parse_bulk_host for kCollateSort (oem_records_stream_push_sort): the same input cut into batches
// at ANY record positions, in any order of the records.  A session cannot sort what it has not seen, so the rule only
// accumulates until finish:
//   - a batch's survivors are its records without OEM_REC_UNMAPPED, in input order; their names (dense, the offsets
//     rebased), their secondary flags (0 for a batch pushed without flags) and their session-global input indices
//     (64-bit: all records of all pushed batches in push order, unmapped ones included) are appended to what is held;
//   - the first surviving record with a bad name (collate_first_bad_name's conditions) is recorded by its
//     session-global index; unmapped records' names are never read;
//   - finish applies parse_bulk_host's sort rule to the held survivors as one cell -- name bytes, primary before
//     secondary, index; a survivor's index among the survivors is ascending in its global index, so rule 3 orders by
//     either -- and cuts the groups where the name changes.  order holds session-global indices.
// The result does not depend on where the batches were cut.
struct ParseBulkSortStream {
    uint64_t n_records = 0, n_unmapped = 0; // of all batches pushed
    std::vector<uint8_t> names;             // the survivors', dense
    std::vector<uint64_t> name_off{0}, global;
    std::vector<uint8_t> secondary;
    uint64_t bad_record = kCollateNoRecord; // session-global; zero_byte tells which
    bool zero_byte = false;
    std::vector<uint64_t> order, group_off; // after finish: n_parsed global indices, n_groups + 1 positions

    template <typename Rec>
    void push(const Rec *records, uint64_t n, const uint8_t *nm, const uint64_t *nm_off, const uint8_t *sec)
    {
        for (uint64_t i = 0; i < n; ++i) {
            if (records[i].flags & kRecUnmapped) {
                ++n_unmapped;
                continue;
            }
            const uint64_t len = nm_off[i + 1] - nm_off[i];
            const bool z = len && memchr(nm + nm_off[i], 0, len);
            if ((!len || z) && bad_record == kCollateNoRecord) {
                bad_record = n_records + i;
                zero_byte = z;
            }
            if (len) names.insert(names.end(), nm + nm_off[i], nm + nm_off[i] + len);
            name_off.push_back(names.size());
            secondary.push_back(sec && sec[i] ? 1 : 0);
            global.push_back(n_records + i);
        }
        n_records += n;
    }
    uint64_t n_parsed() const { return global.size(); }
    void finish()
    {
        const uint64_t m = global.size();
        order.clear();
        group_off.assign(1, 0);
        if (bad_record != kCollateNoRecord || m == 0) return;
        std::vector<uint32_t> pos(m);
        for (uint64_t k = 0; k < m; ++k) pos[k] = (uint32_t)k;
        std::sort(pos.begin(), pos.end(), [&](uint32_t i, uint32_t j) { return collate_before(names.data(), name_off.data(), secondary.data(), i, j); });
        group_off.clear();
        for (uint64_t p = 0; p < m; ++p) {
            const uint32_t i = pos[p], j = p ? pos[p - 1] : 0;
            if (p == 0 || collate_name_cmp(names.data() + name_off[i], name_off[i + 1] - name_off[i], names.data() + name_off[j],
                                           name_off[j + 1] - name_off[j]) != 0)
                group_off.push_back(p);
            order.push_back(global[i]);
        }
        group_off.push_back(m);
    }
};

// Cells from a barcode-collated stream (ParseCellsStream below, oem_cells_stream_push_barcodes): single_cell.rs:196-227
// with alignment_parser.rs:244-299 -- the reference's single-cell driver walks a barcode-collated BAM record by record,
// cuts a cell where the CB tag changes and hands the cell to a worker that sorts it by read name.  The session's input
// is its accepted batches concatenated in ticket order; a record's session-global index (64 bits) counts all records
// of all batches in that order, unmapped ones included.
//   skip     a record with OEM_REC_UNMAPPED takes no part in anything below (alignment_parser.rs:265-288): it cuts no
//            cell and no read, its barcode and its name are never looked at (they may be empty or hold a 0 byte), and
//            n_unmapped counts these records.  The survivors are the other records, in input order.
//   bytes    the survivors' barcodes and names are not empty and hold no 0 byte; the first violation, by the record's
//            session-global index, is an error.
//   cells    a cell is a maximal run of byte-equal barcodes among the survivors.  A barcode that comes back later is a
//            NEW cell with the same label: the reference has no memory of earlier barcodes either.  Cells are numbered
//            in closing order, which is input order.  There is no case folding: the reference uppercases the label
//            (single_cell.rs:206) but compares raw bytes (alignment_parser.rs:153), so lower-case input never
//            terminates there and there is nothing to mirror.
//   NOT reproduced: the reference reads the CB of the peeked record BEFORE it skips unmapped records
//            (single_cell.rs:200-213), so an unmapped record that leads a run under a foreign barcode gives an empty
//            cell there.  Here it gives nothing.
//   inside a cell   the name rule at the top of this file, as it stands: kCollateSort orders by name bytes, primary
//            first, index; kCollateAdjacent only cuts.  The same name in two cells is two groups.
//   stream   the open cell (the carry) is the trailing run of one barcode among all survivors pushed so far;
//            a batch's first run joins it when the barcodes are equal byte for byte, otherwise the carry is closed
//            before the batch's first run; a batch closes every run but its last, which becomes the new carry; a batch
//            without a survivor (an empty batch, a batch of unmapped records only) changes nothing but the counts;
//            finish closes the carry.
// With S the survivors' session-global indices, ascending, the session gives what the one call over the cells
// (oem_em_run_cells_records_names_sparse) gives on R[S], names[S], secondary[S] with the walk's cell_rec_off.
struct ParseCellsStream {
    uint64_t n_records = 0, n_unmapped = 0;        // of all batches pushed
    std::vector<uint64_t> survivors;               // S
    std::vector<uint64_t> cell_rec_off{0};         // positions in S: the closed cells' first survivors, then their end
    std::vector<std::vector<uint8_t>> cell_barcode; // the closed cells' labels
    bool open = false;                             // the carry: its barcode and its size so far
    std::vector<uint8_t> open_barcode;
    uint64_t open_size = 0;

    void close()
    {
        if (!open) return;
        cell_rec_off.push_back(cell_rec_off.back() + open_size);
        cell_barcode.push_back(open_barcode);
        open = false;
        open_size = 0;
    }
    template <typename Rec>
    void push(const Rec *records, uint64_t n, const uint8_t *barcodes, const uint64_t *barcode_off)
    {
        for (uint64_t i = 0; i < n; ++i) {
            if (records[i].flags & kRecUnmapped) {
                ++n_unmapped;
                continue;
            }
            const uint8_t *bc = barcodes + barcode_off[i];
            const uint64_t len = barcode_off[i + 1] - barcode_off[i];
            if (!open || collate_name_cmp(bc, len, open_barcode.data(), open_barcode.size()) != 0) {
                close();
                open = true;
                open_barcode.assign(bc, bc + len);
            }
            ++open_size;
            survivors.push_back(n_records + i);
        }
        n_records += n;
    }
    void finish() { close(); }
};

// Cells from a stream in any order (ParseCellsAnyOrderStream below, oem_cells_stream_set_barcodes_any_order): the barcode
// rule at the top of this file ("Cells from barcodes") applied to a session's input, which is its accepted batches
// concatenated in ticket order; a record's session-global index (64 bits) counts every record of every batch in that
// order, unmapped ones included.
//   skip     a record with OEM_REC_UNMAPPED takes no part: its barcode and name bytes are never examined, so they may be
//            empty or hold a 0 byte.  The other records are the survivors S, ascending.
//   bytes    a survivor's barcode and name are not empty and hold no 0 byte.
//   cells    a cell is the set of survivors with one barcode, compared as bytes.  Cells are numbered by their first
//            survivor in S.  A barcode that comes back is the SAME cell, unlike the collated session above.
//   inside a cell   the survivors keep session order; the name rule (mode) is then applied as it stands.
//   result   finish gives exactly what oem_em_run_cells_records_barcodes_sparse gives on records[S], barcodes[S],
//            names[S], secondary[S], however the input was cut and whichever thread pushed what; `order` is S[order of the
//            one call], 64 bits wide.
//   stream   nothing can run before finish, because any barcode may return.  Per batch the barcodes are INTERNED against
//            the table of the labels seen so far (oem_barcode_table.h): every survivor is looked up; the survivors that
//            miss are sorted by barcode, the runs' heads ranked by survivor index, and the new labels get the ids
//            n_labels + rank -- so ids are first-survivor numbers whatever the cut; the table grows to keep its load at
//            or below 1/2 and takes the new labels; the misses are looked up again.  A survivor keeps its 4-byte cell
//            id; finish sorts the survivors by id, stably.
// The walk below does per batch on the host what the device does per batch.
struct ParseCellsAnyOrderStream {
    uint64_t n_records = 0, n_unmapped = 0, misses = 0; // misses: survivors that missed the first lookup of their batch
    std::vector<uint64_t> survivors;                    // S
    std::vector<uint32_t> cell_id;                      // by survivor
    BarcodeTableHost table;
    uint64_t max_batch_rebuilds = 0;
    // after finish: the survivors' positions in S, cell-major, and the cells' first positions in that order
    std::vector<uint64_t> order, cell_rec_off;

    explicit ParseCellsAnyOrderStream(uint64_t slots0 = kBarcodeTableSlots0, uint32_t hash_bits = 64) : table(slots0, hash_bits) {}

    template <typename Rec>
    void push(const Rec *records, uint64_t n, const uint8_t *barcodes, const uint64_t *barcode_off)
    {
        std::vector<uint64_t> at; // the batch's survivors, as batch indices
        for (uint64_t i = 0; i < n; ++i) {
            if (records[i].flags & kRecUnmapped) ++n_unmapped;
            else at.push_back(i);
        }
        auto bc = [&](uint64_t i) { return barcodes + barcode_off[i]; };
        auto len = [&](uint64_t i) { return barcode_off[i + 1] - barcode_off[i]; };
        // 1. the lookup, against the table as the batch finds it
        const size_t base = cell_id.size();
        std::vector<uint64_t> miss; // positions in `at`
        for (size_t k = 0; k < at.size(); ++k) {
            cell_id.push_back(table.find(bc(at[k]), len(at[k])));
            survivors.push_back(n_records + at[k]);
            if (cell_id.back() == kBarcodeEmpty) miss.push_back(k);
        }
        misses += miss.size();
        if (!miss.empty()) {
            // 2. the distinct barcodes among the misses, numbered by their first survivor
            std::vector<uint64_t> sorted = miss;
            std::stable_sort(sorted.begin(), sorted.end(), [&](uint64_t a, uint64_t b) {
                return collate_name_cmp(bc(at[a]), len(at[a]), bc(at[b]), len(at[b])) < 0;
            });
            std::vector<uint64_t> heads; // a run's head is its first member: its smallest, the sort being stable
            for (size_t p = 0; p < sorted.size(); ++p)
                if (p == 0 || collate_name_cmp(bc(at[sorted[p - 1]]), len(at[sorted[p - 1]]), bc(at[sorted[p]]), len(at[sorted[p]])) != 0)
                    heads.push_back(sorted[p]);
            std::sort(heads.begin(), heads.end());
            const uint64_t first_new = table.n_labels();
            for (uint64_t h : heads) {
                table.labels.insert(table.labels.end(), bc(at[h]), bc(at[h]) + len(at[h]));
                table.label_off.push_back(table.labels.size());
            }
            // 3. / 4. the table grows if it must and takes the new labels
            const uint64_t before = table.rebuilds;
            table.add_from(first_new);
            max_batch_rebuilds = std::max(max_batch_rebuilds, table.rebuilds - before);
            // 5. the misses again
            for (uint64_t k : miss) cell_id[base + k] = table.find(bc(at[k]), len(at[k]));
        }
        n_records += n;
    }
    uint64_t n_cells() const { return table.n_labels(); }
    void finish()
    {
        const uint64_t m = cell_id.size(), nc = n_cells();
        cell_rec_off.assign(nc + 1, 0);
        for (uint64_t k = 0; k < m; ++k) ++cell_rec_off[cell_id[k] + 1];
        for (uint64_t c = 0; c < nc; ++c) cell_rec_off[c + 1] += cell_rec_off[c];
        std::vector<uint64_t> next(cell_rec_off.begin(), cell_rec_off.end() - 1);
        order.assign(m, 0);
        for (uint64_t k = 0; k < m; ++k) order[next[cell_id[k]]++] = k; // stable: session order inside a cell
    }
};

// UMIs in the sessions (oem_cells_stream_set_umis, oem_cells_stream_push_barcodes_umis; oem_cells_barcodes_stream.hip).  A
// UMI session is a barcoded session, of either form above, whose batches carry one UMI byte string per record; the empty
// string means no UB tag.  Cells are cut or interned by the form's own rule, and "UMI deduplication" above is applied
// to every cell behind its name collation.
//   skip     an unmapped record takes no part: its UMI bytes are never examined and may hold a 0 byte.
//   bytes    a surviving record's UMI may be empty; it may not hold a 0 byte.
//   any-order form   with S the survivors' session-global indices, ascending, finish gives exactly what
//            oem_em_run_cells_records_umis_sparse gives on records[S], barcodes[S], names[S], secondary[S], umis[S] with
//            the session's filters, model and mode; `order` is S[order of the one call].
//   collated form    there is no one call to name, because a barcode that comes back is a NEW cell here.  The contract
//            is this join on the S-arrays, with cell_rec_off from the streamed cell rule (maximal runs of byte-equal
//            barcodes): 1. oem_collate_names with that cell_rec_off; 2. oem_dedup_umis on its output with umis[S] and
//            the flags of records[S]; 3. the duplicates' positions dropped (dedup_drop_host); 4.
//            oem_em_run_cells_records_sparse on records[S][order'].  Classes never span cells: two runs of one barcode
//            that hold the same UMI keep both reads.
//   exact    in both forms every index array and count, kept, the discard tables (a duplicate is in none), cell_dups, the
//            labels and the columns equal the expected side's; values and infos as a session is held to its one call --
//            however the input was cut and whichever thread pushed what.  A session all of whose UMIs are empty gives
//            the result of the same session without UMIs, exactly.
//   groups   a session deduplicates group by group (a group is a run of whole cells), on group-local record indices and
//            the group's window of the arena's UMI offsets.  Classes being inside cells, the groups' pieces joined --
//            every later group's positions and read numbers moved down by what the earlier ones lost -- are the
//            whole-input walk's, whatever the groups are (tests/native/cells_umis_stream_main.cpp).
//   counts   the session's cell_rec_off, order and group_off describe the DEDUPLICATED collation: records accepted =
//            unmapped + positions of order + the duplicates' records.
//   bad ref_ids   the sessions differ from the one call and from each other.  The any-order form checks ref_id per batch
//            on every surviving record, as it does without UMIs: a bad ref_id in a record that would later turn out to
//            be a duplicate is still an error there.  The collated form finds it in the group, among the reads that
//            remain: a duplicate's records are never gathered, so its ref_ids are never seen.  (The one call checks
//            among the reads that remain too, but names the cell and the input index instead of a ticket.)  The
//            any-order form's bound of 2^31 - 2 survivors counts the duplicates' records too.

} // namespace oem
