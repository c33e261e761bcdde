// oem_cells.h -- what the one-call per-cell entry points (oem_cells.hip) and the per-cell session
// (oem_cells_stream.hip) share: the sparse blocks of a group, the group itself, the group rule and the result handle.
#pragma once

#include <functional>
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
    // A group filtered from records on the device (oem_cells_records.hip) has no host arrays: `resident` holds the row
    // pointers and the ids, and these are on the device -- the coordinates and probabilities for the coverage model
    // (which then uploads nothing), and a copy of the ids as the filter wrote them, from which a batch the tiler
    // declines gets them back and the host layout builder reads them.
    const uint32_t *d_aln_start = nullptr, *d_aln_end = nullptr;
    const float *d_as_prob = nullptr;
    const uint32_t *d_tid_orig = nullptr;
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
// unless out->row_ptr holds them), the ids and the f64 weights are left in `out`.  With g.d_aln_start set nothing is
// uploaded: out->tid is there already, the coordinates and probabilities are the group's device arrays.
int cells_coverage_group(const CellsCoverage &cc, const CellsGroup &g, ResidentCsr *out);

// oem_cells_records.hip: a group of cells from its alignment records (single_cell.rs:104-188) -- filtered on the device
// into a resident CSR, then run_cells_group on it.  Shared by oem_em_run_cells_records_sparse and the records session.
struct RecordsFilter {
    oem_filters f{};
    std::vector<uint64_t> txp_len;
    std::vector<float> tab; // filter_prob_table of f.score_prob_denom
    bool host_only = false; // no gap table: every group takes the host loop
};
struct RecordsGroup {
    const oem_aln_record *records = nullptr; // the group's records (its first record is records[0])
    bool pinned = false;                     // ... in page-locked memory
    const uint64_t *group_off = nullptr;     // n_groups + 1, from 0
    uint64_t n_groups = 0;
    const uint64_t *cell_group_off = nullptr; // n_cells + 1, from 0 to n_groups
    uint32_t n_cells = 0;
    uint64_t first_cell = 0, first_record = 0; // the group's place in the call or session, for messages
    uint32_t *out_kept = nullptr;            // n_groups, or NULL
    oem_discard_table *out_tables = nullptr; // n_cells
    SparseBlock *blk = nullptr;
    oem_run_info *infos = nullptr;           // n_cells
    LaunchRecord *launch = nullptr;
};
int records_filter_setup(const char *who, const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps, RecordsFilter *rf);
int run_records_group(const char *who, const CellsRun &run, const RecordsFilter &rf, const RecordsGroup &rg, bool *batched);
// cell_group_off: not NULL, from 0, not decreasing, to n_groups
int check_cell_group_off(const char *who, const uint64_t *cell_group_off, uint32_t n_cells, uint64_t n_groups);
// The test-only library's OEM_TEST_KEEP_RECORDS_CSR=1: the filtered CSR of the last group that went through the device
// pass (oem_debug_cells_records_last_csr): dims3 = reads, alignments, cells; any output may be NULL.
int cells_records_last_csr(uint64_t *dims3, uint32_t *row_ptr, uint32_t *tid, uint32_t *as_prob_bits, uint32_t *start,
                           uint32_t *end, uint64_t *cell_row_off);

// oem_cells.hip: the two halves of a per-cell call that its forms share.
// The cut: cells [0, n_cells) into groups of consecutive cells under the group rule, cell c owning entries
// [cell_off[c], cell_off[c + 1]) of `ptr` (reads of a CSR's row pointers, or record groups of their offsets: then the
// bound counts records, which bound the alignments kept); one large group is split head : rest.  ptr = NULL: cell_off
// are record offsets themselves (records that are not cut into reads yet: they bound the reads and the alignments).
std::vector<std::pair<uint32_t, uint32_t>> cut_cells_groups(const uint64_t *cell_off, uint32_t n_cells, const uint64_t *ptr,
                                                            uint32_t n_txps);
// The workers: two host threads (testing build: OEM_CELLS_WORKERS) draw groups from one counter and call
// one(g, run, &path) for each -- it fills path->batched and path->launch; the loops are timed into run.timing.  Leaves
// the record of oem_cells_last_timing and oem_debug_cells_last_paths; the error of the lowest failed group is returned.
int run_cells_workers(const char *who, CellsRun run, const std::vector<std::pair<uint32_t, uint32_t>> &groups,
                      const std::function<int(size_t, const CellsRun &, CellsGroupPath *)> &one);

} // namespace oem

// one call's sparse results (immutable once returned): the groups' blocks in group order -- which is cell order --
// and the cells' offsets; oem_cells_result_copy concatenates the blocks straight into the caller's arrays
struct oem_cells_result {
    uint32_t n_cells = 0;
    uint64_t n_entries = 0;
    std::vector<uint64_t> cell_off; // n_cells + 1
    std::vector<oem::SparseBlock> blocks;
    std::vector<oem_run_info> infos; // n_cells
    // a result that came from records (oem_em_run_cells_records_sparse, a records session): every cell's DiscardTable
    bool from_records = false;
    std::vector<oem_discard_table> discard; // n_cells
};

namespace oem {
// The cells' offsets from the groups' blocks, in group (= cell) order; the blocks move into the result.
int cells_result_from_blocks(const char *who, std::vector<SparseBlock> &blocks, oem_cells_result *r);
// oem_gene_counts.hip: the argument checks of oem_cells_gene_counts (everything but `out`), before any device use, and
// its result from the batches' blocks (infos zero-filled, no discard tables).
int gene_counts_check(const char *who, const uint64_t *cell_off, uint32_t n_cells, const uint32_t *col, const float *val,
                      const uint32_t *gene_of, uint32_t n_txps, uint32_t n_genes);
int gene_counts_result(const char *who, uint32_t n_cells, std::vector<SparseBlock> &blocks, oem_cells_result **out);
} // namespace oem
