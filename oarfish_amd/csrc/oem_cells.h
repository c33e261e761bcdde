// oem_cells.h -- what the one-call per-cell entry points (oem_cells.hip) and the per-cell session
// (oem_cells_stream.hip) share: the sparse blocks of a group, the group rule, the unit of work and the result handle.
#pragma once

#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "oem_driver.h"

namespace oem {

// std::vector storage whose resize leaves new elements default-initialised: a block's entries are written by the
// device read-back, there is no point in zeroing them first
template <typename T>
struct NoInitAlloc : std::allocator<T> {
    template <typename U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <typename U>
    NoInitAlloc(const NoInitAlloc<U> &) noexcept {}
    template <typename U>
    void construct(U *p) noexcept(std::is_nothrow_default_constructible<U>::value) { ::new ((void *)p) U; }
    template <typename U, typename... A>
    void construct(U *p, A &&...a) { ::new ((void *)p) U(std::forward<A>(a)...); }
};

// The sparse results of one group of cells (oem_em_run_cells_sparse): entries per cell, then every cell's columns and
// values one after the other, in cell order.
struct SparseBlock {
    std::vector<uint32_t> counts;
    std::vector<uint32_t, NoInitAlloc<uint32_t>> col;
    std::vector<float, NoInitAlloc<float>> val;
};

// Where the groups of one call put their results: the caller's dense n_cells x n_txps matrix (oem_em_run_cells), or
// one SparseBlock per group index (oem_em_run_cells_sparse: groups finish in any order).
struct CellsSink {
    double *dense = nullptr;
    std::vector<SparseBlock> *blocks = nullptr;
};

// A group whose row pointers are on the device already (the session builds them there from the pushed cells): the
// group has no concatenated host row_ptr unless a fallback asks for one.
struct CellsGroupDevice {
    ResidentCsr *resident = nullptr;           // row_ptr set; without the coverage model also tid and w32
    const unsigned long long *d_cell_row_off = nullptr; // device, n_cells + 1
    const uint64_t *cell_aln_off = nullptr;    // host, n_cells + 1: the cells' first alignments
    const uint32_t *aln_start = nullptr, *aln_end = nullptr; // host, the group's own (coverage model)
    uint64_t nnz = 0;
    uint64_t first_cell = 0;                   // the first cell's number, for messages
};

// The group rule of the per-cell driver: may `cells` consecutive cells with `reads` reads and `gnnz` alignments be
// one batched store (transcript space < 2^32, the alignment bound, the layout builder's tile x bucket table)?
bool cells_group_fits(uint64_t cells, uint64_t reads, uint64_t gnnz, uint32_t n_txps, uint64_t max_group_nnz);
uint64_t cells_max_group_nnz(); // the alignment bound of a group (testing build: OEM_CELLS_GROUP_NNZ)

// One group of consecutive cells [c0, c1): batched on the device when it can be, otherwise cell after cell.  With
// `dev` (c0 = 0, row_ptr NULL) the group's CSR is resident already.
int run_cells_group(const uint64_t *cell_row_off, uint32_t c0, uint32_t c1, const uint64_t *row_ptr,
                    const uint32_t *tid, const float *as_prob, const double *cov_prob, const CellsCoverage *cov_src,
                    uint32_t n_txps, int device, uint32_t max_iter, double conv_thresh, const CellsSink &sink, size_t g,
                    oem_run_info *infos, bool *batched, const CellsGroupDevice *dev = nullptr);

} // namespace oem

// one call's sparse results (immutable once returned): the groups' blocks in group order -- which is cell order --
// and the cells' offsets; oem_cells_result_copy concatenates the blocks straight into the caller's arrays
struct oem_cells_result {
    uint32_t n_cells = 0;
    uint64_t n_entries = 0;
    std::vector<uint64_t> cell_off; // n_cells + 1
    std::vector<oem::SparseBlock> blocks;
    std::vector<oem_run_info> infos; // n_cells
};

namespace oem {
// The cells' offsets from the groups' blocks, in group (= cell) order; the blocks move into the result.
int cells_result_from_blocks(const char *who, std::vector<SparseBlock> &blocks, oem_cells_result *r);
} // namespace oem
