// oem_gene_counts.h -- the cells x transcripts matrix collapsed to cells x genes, as a pure host function.
//
// Nothing of this is in the reference, which writes cells x transcripts only (write_function.rs:53-54).  The rule is
// stated here once; the kernels of oem_gene_counts.hip, the host walk below (the testing library's
// oem_test_cells_gene_counts_host, the stand-alone program of tests/test_gene_counts.py) and the documentation of
// oem_cells_gene_counts all refer to this file.
//
// Input: a CSR of n_cells cells (cell_off, col, val: what oem_em_run_cells_sparse and the sessions return) and gene_of,
// one gene id per transcript.
//   run       for cell c and gene g: the entries of cell c whose gene_of[col] is g, in CSR order.
//   sum       the run's values, each converted to f64, added one after the other in that order, starting from 0.0; the
//             sum is rounded ONCE to f32, to nearest-even, denormals kept (__double2float_rn, Rust's `as f32`).
//   entry     cell c has an entry for gene g iff the run is not empty.  There is no test on the value: a run of +0.0
//             entries gives an entry of +0.0, and a sum beyond the f32 range gives +inf.
//   order     a cell's entries come in ascending gene id.
// The input values are taken as they are.  With the project's CSRs (ascending transcript, v > 0) a run is "the gene's
// transcripts expressed in the cell, in ascending id".  gene_of need not be monotone and gene ids may have gaps.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace oem {

constexpr uint64_t kGeneMaxCellEntries = 1ull << 30; // entries of one cell (the device sort and scan count in int)
constexpr uint64_t kGeneBatchEntries = 1ull << 27;   // entries of a batch of cells (the test-only library: OEM_GENE_BATCH_ENTRIES)

// The host walk of the rule: the specification.  counts (n_cells: the cells' gene entries), gene and out_val (their sum)
// are overwritten.  The arguments are checked by the caller.
template <typename GeneVec, typename ValVec>
inline void gene_counts_host(const uint64_t *cell_off, uint32_t n_cells, const uint32_t *col, const float *val,
                             const uint32_t *gene_of, std::vector<uint32_t> *counts, GeneVec *gene, ValVec *out_val)
{
    counts->assign(n_cells, 0);
    gene->clear();
    out_val->clear();
    std::vector<std::pair<uint32_t, uint64_t>> ent; // (gene, entry) of one cell
    for (uint32_t c = 0; c < n_cells; ++c) {
        ent.clear();
        for (uint64_t e = cell_off[c]; e < cell_off[c + 1]; ++e) ent.emplace_back(gene_of[col[e]], e);
        // stable: inside a gene the entries keep CSR order
        std::stable_sort(ent.begin(), ent.end(), [](const std::pair<uint32_t, uint64_t> &a, const std::pair<uint32_t, uint64_t> &b) { return a.first < b.first; });
        for (size_t k = 0; k < ent.size();) {
            double acc = 0.0;
            size_t j = k;
            for (; j < ent.size() && ent[j].first == ent[k].first; ++j) acc += (double)val[ent[j].second];
            gene->push_back(ent[k].first);
            out_val->push_back((float)acc);
            ++(*counts)[c];
            k = j;
        }
    }
}

} // namespace oem
