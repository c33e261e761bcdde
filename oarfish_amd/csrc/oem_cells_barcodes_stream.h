// oem_cells_barcodes_stream.h -- what the per-cell session (oem_cells_stream.hip) and its barcoded form
// (oem_cells_barcodes_stream.hip) share: what a group leaves for the session's result, what the barcoded part asks of
// the session it belongs to, and the calls between the two.  The rule is oem_collate.h's "Cells from a barcode-collated
// stream".
#pragma once

#include <functional>
#include <string>
#include <vector>

#include "oem_cells.h"
#include "oem_collate.h"
#include "oem_filter_device.h"

namespace oem {

// what one group of a session leaves: its sparse block, its cells' infos and, from records, their discard tables
struct StreamGroupResult {
    SparseBlock blk;
    std::vector<oem_run_info> infos;
    std::vector<oem_discard_table> tables;
};
// a group that runs from device memory: called once on one of the session's group workers, or destroyed unrun when the
// session is stuck or cancelled
using StreamGroupRun = std::function<int(StreamGroupResult *, bool *batched)>;

// The session as its barcoded part sees it.  The callbacks take the session's lock: none is called with the barcoded
// part's own lock held.
struct BarcodesEnv {
    uint32_t n_txps = 0;
    int device = 0;
    uint32_t max_iter = 0;
    double conv_thresh = 0.0;
    CellsCoverage *cov = nullptr;      // the session's coverage model, or NULL
    const RecordsFilter *rf = nullptr; // the session's filters
    uint64_t group_nnz = 0, max_staged = 0; // counted in records
    uint32_t group_cells = 0;
    uint32_t mode = kCollateSort;
    std::function<void(StreamGroupRun)> submit;        // the next group, in cell order, to the group workers
    std::function<void(int, const char *)> set_sticky; // the first error sticks
    std::function<int(std::string *)> sticky;          // OEM_OK, or the session's sticky status and its message
    std::function<void(uint64_t)> add_blocked_us;
};

struct BarcodesStream;
int barcodes_stream_create(const BarcodesEnv &env, BarcodesStream **out);
// oem_cells_stream_push_barcodes behind its NULL-session check
int barcodes_stream_push(BarcodesStream *b, const char *who, const oem_aln_record *records, uint64_t n_records, const uint8_t *barcodes,
                         const uint64_t *barcode_off, const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary,
                         uint64_t *out_ticket);
bool barcodes_stream_push_in_flight(BarcodesStream *b);
// finish, before the group workers are stopped: no further push is accepted, the staged batches are parsed, the open
// cell is closed and what the arena still holds goes to the workers
int barcodes_stream_close(BarcodesStream *b, const char *who);
// finish, after the group workers have joined: the groups' pieces become what oem_cells_stream_barcodes_copy gives
int barcodes_stream_assemble(BarcodesStream *b, const char *who);
void barcodes_stream_counts(BarcodesStream *b, uint64_t *n_batches, uint64_t *n_records);
int barcodes_stream_dims(const BarcodesStream *b, const char *who, uint64_t *n_cells, uint64_t *n_survivors, uint64_t *n_groups,
                         uint64_t *barcode_bytes, uint64_t *n_unmapped);
int barcodes_stream_copy(const BarcodesStream *b, const char *who, uint8_t *out_barcodes, uint64_t *out_barcode_off,
                         uint64_t *out_cell_rec_off, uint64_t *out_order, uint64_t *out_group_off, uint64_t *out_cell_group_off,
                         uint32_t *out_kept);
// stops the parse worker (staged batches are dropped) and frees everything; the session's group workers have joined
void barcodes_stream_destroy(BarcodesStream *b);
// destroy's first half, before the session's group workers are joined: nothing more is parsed or submitted
void barcodes_stream_cancel(BarcodesStream *b);

// oem_cells_records.hip: a group of cells behind its device filter pass (consumes r), and the host loop of a group
int records_group_filtered(const CellsRun &run, const RecordsGroup &rg, FilterResult &r, FilterCells &fc, bool *batched);
int records_group_host(const char *who, const CellsRun &run, const RecordsFilter &rf, const RecordsGroup &rg, bool *batched);

} // namespace oem
