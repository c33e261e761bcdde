// oem_cells_barcodes_stream.h -- what the per-cell session (oem_cells_stream.hip) and its barcoded form
// (oem_cells_barcodes_stream.hip) share: what a group leaves for the session's result, what the barcoded part asks of
// the session it belongs to, and the calls between the two.  The rule is oem_collate.h's "Cells from a barcode-collated
// stream" or, for the any-order form (oem_cells_barcodes_sort_stream.hip), "Cells from a stream in any order".
#pragma once

#include <functional>
#include <string>
#include <vector>

#include "oem_cells.h"
#include "oem_collate.h"
#include "oem_collate_device.h"
#include "oem_dev_blob.h"
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
};

// The any-order session's table of the labels seen so far, on the device (oem_cells_barcodes_sort_stream.hip,
// oem_barcode_table.h): its slots, the labels in id order (a DevBlob, oem_dev_blob.h), and what it counts.
// Everything runs on the null stream and leaves it idle.
struct BarcodeIntern {
    DevBuf<uint32_t> slot;
    DevBlob labels;
    DevBuf<unsigned long long> stats; // the kernels' words: the longest probe, a probe wrapped, an error
    uint64_t capacity = 0;
    uint32_t hash_bits = 64;
    uint64_t misses = 0, rebuilds = 0, max_doublings = 0, longest_probe = 0;
    bool wrapped = false;

    int init(); // the first capacity (the testing library: OEM_BARCODE_TABLE_SLOTS0, OEM_BARCODE_HASH_BITS)
    void release();
    // One batch: its m survivors' barcodes as a dense checked blob (8-byte aligned, padded by 16) with m + 1 offsets
    // from 0 -> d_cell_id[0 .. m), the cells' numbers.  New labels are numbered by their first survivor.
    int batch(const char *who, const uint8_t *d_bc, const uint64_t *d_bc_off, uint64_t m, uint32_t *d_cell_id);
    // finish: order_bc and cell_rec_off of n > 0 survivors from their cell ids, by one stable radix sort
    int cells(const uint32_t *d_cell_id, uint64_t n, BarcodeCells *out);
    int labels_down(std::vector<uint8_t> *out_labels, std::vector<uint64_t> *out_label_off);
    void publish_last() const; // what oem_debug_barcode_table_last reports
    int check_stats(const char *who);
};
// the last finished any-order session's table (8 words): [0] rebuilds, [1] the longest probe, [2] a probe wrapped past the
// table's end, [3] the most doublings one rebuild covered, [4] the final capacity, [5] labels, [6] misses
void barcode_table_last(uint64_t *out8);
// k_barcode_insert for a table that is built elsewhere (the whitelist of oem_barcode_correct.hip): the labels [first,
// first + cnt) of a padded label blob, distinct or not, into the first free slots of their probe paths.  d_stats: three
// words -- the longest probe, a probe wrapped, a probe went round the table.  Queued on the null stream.
int barcode_table_insert(uint64_t first, uint64_t cnt, uint32_t *d_slot, uint64_t capacity, uint32_t hash_bits, const uint8_t *d_labels,
                         const uint64_t *d_label_off, unsigned long long *d_stats);
// d_out[k] = d_in[0] + ... + d_in[k - 1] over n entries, in 64 bits (oem_cells_barcodes_stream.hip); leaves the null stream idle
int exclusive_scan_u32(const uint32_t *d_in, uint64_t *d_out, uint64_t n);

struct BarcodesStream;
// any_order: oem_collate.h's "Cells from a stream in any order" instead of "Cells from a barcode-collated stream"
int barcodes_stream_create(const BarcodesEnv &env, bool any_order, BarcodesStream **out);
// what oem_cells_stream_info reports of an any-order session (0 for a collated one): the arena's peak in bytes, the
// survivors that missed the first lookup of their batch, the table's capacity
void barcodes_stream_table_info(BarcodesStream *b, uint64_t *arena_peak, uint64_t *misses, uint64_t *slots);
// oem_cells_stream_push_barcodes and (with_umis) oem_cells_stream_push_barcodes_umis behind their NULL-session check: the
// call that does not belong to the session's kind is OEM_ERR_STATE
int barcodes_stream_push(BarcodesStream *b, const char *who, const oem_aln_record *records, uint64_t n_records, const uint8_t *barcodes,
                         const uint64_t *barcode_off, const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary,
                         bool with_umis, const uint8_t *umis, const uint64_t *umi_off, uint64_t *out_ticket);
// oem_cells_stream_set_umis behind its checks of the session: before any push, once (oem_collate.h, "UMIs in the sessions")
int barcodes_stream_set_umis(BarcodesStream *b, const char *who);
// the duplicates dropped by the groups that have run: reads, and their records (0 without UMIs)
// ... and, under a rule with correct, the reads corrected
void barcodes_stream_umi_info(BarcodesStream *b, uint64_t *dup_reads, uint64_t *dup_records, uint64_t *corrected_reads);
// oem_cells_stream_set_umi_rule behind its NULL-session check: after set_umis, before any push, once; gene_of is copied
// and uploaded to the session's device (oem_collate.h, "The UMI rule")
int barcodes_stream_set_umi_rule(BarcodesStream *b, const char *who, const oem_umi_rule *rule);
// oem_cells_stream_umi_rule_copy: the reads corrected in every cell, after finish of a session whose rule has correct
int barcodes_stream_umi_rule_copy(const BarcodesStream *b, const char *who, uint64_t *out_cell_corrected);
// oem_cells_stream_set_whitelist behind its NULL-session check: an any-order session, before any push, once; the rule's
// arrays are copied and its whitelist is built on the session's device (oem_barcode_correct.h, "The rule in a session")
int barcodes_stream_set_whitelist(BarcodesStream *b, const char *who, const oem_barcode_rule *rule);
// oem_cells_stream_whitelist_copy: every cell's whitelist id and corrected records, and the five status counts, after
// finish of a whitelist session; each output or NULL
int barcodes_stream_whitelist_copy(const BarcodesStream *b, const char *who, uint32_t *out_cell_wl_id, uint64_t *out_cell_bc_corrected,
                                   uint64_t *out_counts);
// the mapped records a whitelist session dropped (per batch or at finish) and those that waited for finish
void barcodes_stream_whitelist_info(BarcodesStream *b, uint64_t *rejected, uint64_t *deferred);
// oem_cells_stream_umis_copy: the duplicates (reads) every cell lost, after finish
int barcodes_stream_umis_copy(const BarcodesStream *b, const char *who, uint64_t *out_cell_dups);
bool barcodes_stream_push_in_flight(BarcodesStream *b);
// finish, before the group workers are stopped: no further push is accepted, the staged batches are parsed, the open
// cell is closed and what the arena still holds goes to the workers
int barcodes_stream_close(BarcodesStream *b, const char *who);
// finish, after the group workers have joined: the groups' pieces become what oem_cells_stream_barcodes_copy gives
int barcodes_stream_assemble(BarcodesStream *b, const char *who);
// batches and records pushed, and the microseconds its pushes have waited for room in the staging budget
void barcodes_stream_counts(BarcodesStream *b, uint64_t *n_batches, uint64_t *n_records, uint64_t *blocked_us);
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
