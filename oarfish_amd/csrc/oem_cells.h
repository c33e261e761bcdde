// oem_cells.h -- what the one-call per-cell entry points (oem_cells.hip) and the per-cell session
// (oem_cells_stream.hip) share: the sparse blocks of a group, the group itself, the group rule and the result handle.
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

struct CellsTiming; // oem_cells.hip: where the groups' EM loops are recorded (oem_cells_last_timing)
// What all groups of a call or a session run with.
struct CellsRun {
    uint32_t n_txps = 0;
    int device = 0;
    uint32_t max_iter = 0;
    double conv_thresh = 0.0;
    CellsCoverage *cov = nullptr;  // the per-cell coverage model as the source of the weights, or NULL
    CellsTiming *timing = nullptr; // or NULL: the loops are not recorded
};

// A group of consecutive cells, the unit of work of the per-cell driver.  Two producers: the one-call form slices it
// out of the caller's arrays (oem_cells.hip: slice_cells), the session fills it from its staging (oem_cells_stream.hip:
// run_group).  Offsets are relative to the group, arrays and results start at its first cell; what is not there is NULL.
struct CellsGroup {
    uint32_t n_cells = 0;
    uint64_t n_reads = 0, nnz = 0, first_cell = 0; // (first_cell: its number in the call or session, for messages)
    const uint64_t *cell_row_off = nullptr, *cell_aln_off = nullptr; // host, n_cells + 1: the cells' first reads / alignments
    const uint64_t *row_ptr = nullptr;      // host, n_reads + 1, or NULL: the u32 row pointers are in `resident` already
    const uint32_t *tid = nullptr;          // host, nnz
    const float *as_prob = nullptr;
    const double *cov_prob = nullptr;       // a host coverage column, or NULL
    const uint32_t *aln_start = nullptr, *aln_end = nullptr; // host (coverage model)
    double *out_cov_prob = nullptr;         // host: the group's part of the caller's coverage column, or NULL
    ResidentCsr *resident = nullptr;        // set: the store adopts it instead of uploading (coverage model, session)
    const unsigned long long *d_cell_row_off = nullptr; // cell_row_off on the device already, or NULL
    double *out_dense = nullptr;            // the results: the group's rows of the caller's n_cells x n_txps matrix,
    SparseBlock *blk = nullptr;             // ... or its sparse block
    oem_run_info *infos = nullptr;          // n_cells, or NULL
    LaunchRecord *launch = nullptr;         // or NULL; a batched group leaves its store's record of the last launches here
};

// The group rule of the per-cell driver: may `cells` consecutive cells with `reads` reads and `gnnz` alignments be
// one batched store (transcript space < 2^32, the alignment bound, the layout builder's tile x bucket table)?
bool cells_group_fits(uint64_t cells, uint64_t reads, uint64_t gnnz, uint32_t n_txps, uint64_t max_group_nnz);
uint64_t cells_max_group_nnz(); // the alignment bound of a group (testing build: OEM_CELLS_GROUP_NNZ)

// One group: batched on the device when it can be, otherwise cell after cell (*batched says which).
int run_cells_group(const CellsRun &run, const CellsGroup &g, bool *batched);
// oem_coverage_cells.hip: the group's coverage on the device from its own arrays; the row pointers (uploaded here
// unless out->row_ptr holds them), the ids and the f64 weights are left in `out`.
int cells_coverage_group(const CellsCoverage &cc, const CellsGroup &g, ResidentCsr *out);

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
