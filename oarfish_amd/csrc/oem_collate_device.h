// oem_collate_device.h -- the resident form of the name collation (oem_collate_device.hip): one batch of cells collated
// on the device, its order and offsets LEFT there.  oem_collate_names copies them to the caller's arrays;
// oem_em_run_cells_records_names_sparse (oem_cells_records.hip) gathers and filters the records behind them instead.
#pragma once

#include <vector>

#include "oem_collate.h"
#include "oem_driver.h"

namespace oem {

// One call's input, as oem_collate_names takes it (already checked), and how the batches are run.
struct CollateInput {
    const char *who = nullptr;   // for the messages of the device-found errors
    const uint8_t *names = nullptr;
    const uint64_t *name_off = nullptr;
    const uint8_t *secondary = nullptr;
    const uint64_t *cell_rec_off = nullptr;
    uint32_t mode = kCollateSort;
    uint64_t chunk_bytes = 0;    // name bytes per upload chunk
    bool timing = false;
    bool cut_records = false;    // the upload chunks may end inside a cell (sorting without secondary only: one cell of everything)
    const char *what = "name";   // what the bytes are called in the device-found errors ("barcode": oem_collate_barcodes)
    // The device form (the groups of oem_em_run_cells_records_barcodes_sparse): the batch's names are on the device
    // already, checked when they went up.  d_names: the batch's blob, 8-byte aligned and padded by 16; d_name_off: the
    // batch's m + 1 offsets into it, d_off_base to be subtracted; d_secondary (or NULL): m flags and a 0 behind them.
    // names / name_off / secondary above are then not read, and there are no upload lanes and no validate pass.
    const uint8_t *d_names = nullptr;
    const uint64_t *d_name_off = nullptr;
    uint64_t d_off_base = 0, d_n_bytes = 0;
    const uint8_t *d_secondary = nullptr;
};

// What a batch leaves on the device.  The batch holds the cells [c0, c1) and their m records.
struct CollateResident {
    DevBuf<uint32_t> order;          // m: order[k] = order_base + the record of the batch at position k
    DevBuf<uint64_t> group_off;      // m + 1 allocated, n_groups + 1 filled: pos_base + the positions where a read starts, then pos_base + m
    DevBuf<uint64_t> cell_group_off; // (c1 - c0) + 1: group_base + the cells' first groups
    uint64_t n_groups = 0;
};

// The cells [c0, c1) of the call, m > 0 records.  The bases are added on the device: oem_collate_names passes the batch's
// place in the call for all three, a caller that goes on working on the batch passes 0 for the positions and groups.  A
// name error names the record by its index in the call, whatever the bases.  info (8 doubles, collate_last_call's
// layout) is accumulated.  Returns with the device idle and the scratch of the sort released.
int collate_resident(const CollateInput &in, uint32_t c0, uint32_t c1, uint64_t order_base, uint64_t pos_base, uint64_t group_base,
                     double *info, CollateResident *out);

// The cells of uncollated records, left on the device (collate_barcodes_resident): order_bc and cell_rec_off of
// oem_collate.h's barcode rule.
struct BarcodeCells {
    DevBuf<uint32_t> order;        // n_records: order_bc
    DevBuf<uint64_t> cell_rec_off; // n_cells + 1
    uint64_t n_cells = 0;
};

// The barcodes of n_records > 0 records (checked by check_barcode_input) sorted as one cell by the key rounds of
// collate_resident, then the runs ranked by their first record and laid out in that rank.  An empty barcode or a 0 byte
// is OEM_ERR_ARG naming the first such record.  info: collate_last_call's layout, accumulated; info8 (8 doubles): [0]
// the cells' kernels in ms under `timing`.  Returns with the device idle.
int collate_barcodes_resident(const char *who, const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n_records, bool timing,
                              double *info, double *cells_ms, BarcodeCells *out);
// The same on barcodes that are on the device already and checked (the misses of a batch of the any-order barcoded
// session, oem_cells_barcodes_sort_stream.hip): a dense blob, 8-byte aligned and padded by 16, with its n_records + 1
// offsets from 0.  out_heads (or NULL): the cells' first records, ascending -- cell c's label is that record's barcode.
int collate_barcodes_device(const char *who, const uint8_t *d_barcodes, const uint64_t *d_barcode_off, uint64_t n_bytes, uint64_t n_records,
                            BarcodeCells *out, DevBuf<uint32_t> *out_heads);
// The argument checks of oem_collate_barcodes on the input side, before any device use.
int check_barcode_input(const char *who, const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n_records);
// The tail of the two calls above, for runs that come from elsewhere (the corrected barcodes, oem_barcode_correct.hip):
// d_sorted holds n positions' records run by run, input order inside a run; d_run_off (n_runs + 1, from 0) the runs'
// first positions; every record is below n_input.  The runs are ranked by their first record and laid out in that rank.
// On the null stream, which is left idle.
int barcode_cells_from_runs(uint64_t n, uint64_t n_runs, uint64_t n_input, const uint32_t *d_sorted, const uint64_t *d_run_off,
                            BarcodeCells *out, DevBuf<uint32_t> *out_heads);

// ---- barcode correction against a whitelist (oem_barcode_correct.hip; the rule is oem_barcode_correct.h's)
// The whitelist of a call on the device: its labels as a padded blob, the table over them, n(w), and the rule's words.
struct BarcodeWhitelist {
    DevBuf<uint32_t> slot, count;    // capacity slots; n_labels counts, 0 until a call's exact pass
    DevBuf<uint8_t> labels;          // padded by 16
    DevBuf<uint64_t> label_off;      // n_labels + 1
    DevBuf<unsigned long long> bad;  // the kernels' error words
    uint64_t capacity = 0, n_labels = 0, len_mask = 0, alphabet = 0; // alphabet: its bytes as one word, byte 0 in the low bits
    uint32_t n_alphabet = 0, multi = 0, hash_bits = 64;
};
// What correct_barcodes_resident leaves on the device: id and status of every record, and the cells of the accepted ones
// (cells.order: n_accepted input indices; cells.cell_rec_off: n_cells + 1 positions).  With n_accepted == 0 there are no
// cells and cells' buffers are empty.
struct CorrectedCells {
    BarcodeCells cells;
    DevBuf<uint32_t> id;
    DevBuf<uint8_t> status;
    uint64_t n_accepted = 0, n_misses = 0, counts[5] = {0, 0, 0, 0, 0}; // counts: by status (kBarcodeStatuses)
};
// oem_correct_barcodes' checks of its rule before any device use
int check_barcode_rule(const char *who, const oem_barcode_rule *rule);
// The checked rule's whitelist up and its table built; a label with a 0 byte and two equal labels are OEM_ERR_ARG.
int whitelist_build(const char *who, const oem_barcode_rule *rule, BarcodeWhitelist *wl);
// The barcodes of n_records records (checked by check_barcode_input) against the whitelist; a barcode with a 0 byte is
// OEM_ERR_ARG naming the smallest such record, an empty one is kBarcodeMissing.  One call per BarcodeWhitelist: n(w) is
// counted into it.  Returns with the device idle and only `out` held.
int correct_barcodes_resident(const char *who, const BarcodeWhitelist &wl, const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n,
                              CorrectedCells *out);
// The tail of correct_barcodes_resident, shared with a whitelist session's finish: the cells of the records whose d_id is
// not kBarcodeNoId -- an accepted flag, a scan, (id & mask, record) compacted, one stable radix sort over the bits
// n_labels needs, the runs ranked by their first record (barcode_cells_from_runs).  *n_accepted: the records in cells;
// m_expected: what it must be, or ~0.  Leaves the null stream idle.
int barcode_cells_from_ids(const char *who, const uint32_t *d_id, uint32_t mask, uint64_t n, uint64_t n_labels, uint64_t m_expected,
                           BarcodeCells *cells, uint64_t *n_accepted);

// ---- the rule in a session (oem_barcode_correct.h, "The rule in a session"; oem_cells_stream_set_whitelist)
// What a batch of a whitelist session leaves: its RETAINED records (accepted or deferred) as the batch's survivor list
// compacted to them with their ids (kBarcodeCorrectedBit on a corrected record, kBarcodeNoId on a deferred one), the
// deferred records' barcodes as a dense padded blob with their arena positions, both in batch order, and the batch's
// final statuses by count (a deferred record is in none).
struct WhitelistBatch {
    DevBuf<uint32_t> order, id;       // n_retained
    DevBuf<uint32_t> deferred_pos;    // n_deferred: arena_n + the record's rank among the retained
    DevBuf<uint8_t> deferred_bc;      // their barcodes ...
    DevBuf<uint64_t> deferred_off;    // ... n_deferred + 1 offsets from 0
    uint64_t n_retained = 0, n_deferred = 0, deferred_bytes = 0, counts[5] = {0, 0, 0, 0, 0};
};
// One batch: the m mapped records d_order[0 .. m) with their barcodes as a dense blob (checked for 0 bytes, padded by 16,
// m + 1 offsets from 0; an empty barcode is legal).  k_bc_exact against the session's n(w), which grows; the neighbour
// pass that decides or defers (k_bc_neighbours_stream); the compaction to the retained records.  arena_n: the arena's
// records before the batch.  Leaves the null stream idle.
int whitelist_batch(const char *who, const BarcodeWhitelist &wl, const uint8_t *d_bc, const uint64_t *d_bc_off, const uint32_t *d_order, uint64_t m,
                    uint64_t arena_n, WhitelistBatch *out);
// finish: the neighbour pass over the pending list with n(w) complete; the winners' ids go to the arena's id column
// (arena_n entries) at their positions, counts (5) are the pending records' statuses.
int whitelist_finish(const char *who, const BarcodeWhitelist &wl, const uint8_t *d_pending, const uint64_t *d_pending_off,
                     const uint32_t *d_pending_pos, uint64_t n_pending, uint32_t *d_arena_id, uint64_t arena_n, uint64_t *counts);
// every cell's whitelist id and the number of its records that were corrected, from the arena's id column
int whitelist_cell_summary(const BarcodeCells &cells, const uint32_t *d_arena_id, std::vector<uint32_t> *cell_label,
                           std::vector<uint64_t> *cell_corrected);

// The records d_order[0 .. m) of a resident padded blob with its offsets: bad2[0] = the smallest with a 0 byte, bad2[1] =
// the smallest without a byte, ~0 where there is none.  The records that are not in d_order are not looked at.
int validate_records_of(const uint32_t *d_order, uint64_t m, const uint8_t *d_blob, const uint64_t *d_off, unsigned long long *bad2);

// The names of the records order[0 .. m) (indices into the whole input's d_name_off, n + 1 offsets into d_names, which
// is 8-byte aligned and padded) gathered into one dense blob: d_out_off (m + 1, from 0: the scan of the lengths, filled
// by gather_name_offsets) and d_out (8-byte aligned, out_bytes + 16 allocated) by gather_names, which takes any window
// [k0, k1) of the records whose offsets are d_out_off[k0 .. k1] - off_base.  d_sec / d_out_sec: the flags likewise
// (d_out_sec: m + 1 rounded up to 8, zero behind the m flags), or NULL.  On the null stream, which is left idle.
// with_empty: some of the names may be empty (a session's UMIs); without it every name holds a byte at least.
int gather_name_offsets(const uint32_t *d_order, uint64_t m, const uint64_t *d_name_off, uint64_t *d_out_off);
int gather_names(const uint32_t *d_order, uint64_t m, const uint8_t *d_names, const uint64_t *d_name_off, const uint64_t *d_out_off,
                 uint64_t off_base, uint64_t out_bytes, uint8_t *d_out, const uint8_t *d_sec, uint8_t *d_out_sec, bool with_empty = false);
// Validates names that are resident (the blob 16-byte padded): the first record with a 0 byte -> d_bad[0], with an empty
// name -> d_bad[1] (both start as kNoRecord), over the records [r0, r1) and their bytes [b0, b1), on `st`.
void launch_collate_validate(hipStream_t st, const uint8_t *d_names, uint64_t b0, uint64_t b1, const uint64_t *d_off, uint64_t r0,
                             uint64_t r1, unsigned long long *d_bad);

// The last oem_collate_barcodes / oem_em_run_cells_records_barcodes_sparse of this thread (8 doubles): [0] key rounds,
// [1] upload chunks of the barcodes, [2] the cells' kernels (ms), [3] the barcode uploads, [4] their chunk kernels, [5]
// the rounds, [6] staging (ms, under OEM_COLLATE_TIMING), [7] the rounds that sorted.
void collate_barcodes_last_call(double *out8);
void collate_barcodes_set_last(const double *in8);
// The last oem_em_run_cells_records_barcodes_sparse of this thread (8 doubles): [0] cells, [1] groups of cells, and by
// the host clock in ms [2] the barcode collation, [3] names, flags and records going up, [4] the gathered name offsets,
// [5] the groups on their workers; under OEM_COLLATE_TIMING from HIP events [6] the name uploads, [7] the validate kernels.
void cells_barcodes_last_call(double *out8);

// oem_cells_records.hip: the caller's records [0, m) into d through the upload lanes; order[k] = outer[order[k]]
// (k_order_compose); dst[k] = src[order[k]] over 40-byte records (k_records_gather).  The last two run on the null
// stream and leave it idle.
int upload_records(const oem_aln_record *records, uint64_t m, oem_aln_record *d);
int order_compose(uint64_t m, const uint32_t *d_outer, uint32_t *d_order);
int records_gather(uint64_t m, const uint32_t *d_order, const oem_aln_record *d_src, oem_aln_record *d_dst);

// ---- UMI deduplication (oem_dedup_umis.hip; the rule is oem_collate.h's)
// The whole input's UMIs and flags on the device, in input order.
struct UmiInput {
    const char *who = nullptr;           // for the messages of the collation over the UMIs
    const uint8_t *d_umis = nullptr;     // the blob, 8-byte aligned and padded by 16
    const uint64_t *d_umi_off = nullptr; // n_records + 1
    const uint32_t *d_flags = nullptr;   // record i's flags word at d_flags[i * flags_stride], or NULL: none unmapped
    uint64_t flags_stride = 1;           // (10 with the flags read out of resident 40-byte records)
    // The UMI rule (oem_collate.h); with d_gene_of == NULL and correct == 0 dedup_mark launches what it launches without.
    const uint32_t *d_ref_id = nullptr;  // record i's ref_id at d_ref_id[i * ref_id_stride]: required with d_gene_of
    uint64_t ref_id_stride = 1;          // (10: word 0 of resident 40-byte records)
    const uint32_t *d_gene_of = nullptr; // n_txps gene ids, or NULL: no gene in the key
    uint32_t n_txps = 0;
    uint32_t correct = 0;                // 1: one-mismatch correction
    // A caller that knows the records' origin (a session's group) words the error of a bad ref_id itself: dedup_mark then
    // returns OEM_OK with UmiMarks::bad_ref_record set and nothing else filled, as filter_device_resident does.
    bool defer_bad_ref = false;
};
// What dedup_mark leaves on the device for a batch of ng groups.
struct UmiMarks {
    DevBuf<uint32_t> dup;      // ng: 0 / 1
    DevBuf<uint64_t> survivor; // ng: survivor_base + the survivor's group
    DevBuf<uint64_t> keep;     // ng + 1: 1 - dup, then 0
    DevBuf<uint64_t> gscan;    // ng + 1, only with n_dups > 0: the exclusive scan of keep, the kept groups' new numbers
    uint64_t n_part = 0, n_classes = 0, n_dups = 0; // (n_classes: only when two groups or more take part)
    // under a rule with correct: the classes that have a parent, the rounds of pointer jumping, and the longest walk of
    // a class over its half-sharing neighbours in the first and in the second (halves swapped) collation
    uint64_t n_corrected_classes = 0, jump_rounds = 0, walk_max[2] = {0, 0};
    // with UmiInput::defer_bad_ref: the smallest input index of the batch that heads a group that takes part and whose
    // ref_id is not below n_txps, and that ref_id (kCollateNoRecord: none)
    uint64_t bad_ref_record = kCollateNoRecord;
    uint32_t bad_ref_id = 0;
};
// The UMIs (checked: umi_off from 0, non-decreasing) up through the upload lanes, validated behind their chunks: a 0 byte
// is OEM_ERR_ARG naming the smallest such input index, an empty UMI is legal.  validate == false: nothing is looked at
// (the whitelist call, which validates the accepted records only; raw barcodes, which their own kernel checks).
int umis_upload(const char *who, const uint8_t *umis, const uint64_t *umi_off, uint64_t n, DevBuf<uint8_t> *d_umis, DevBuf<uint64_t> *d_umi_off,
                bool validate = true);
// A session's batch (oem_cells_barcodes_stream.hip), whose UMIs are resident (d_umis padded by 16, n + 1 offsets): the
// UMIs of the m > 0 survivors d_order[0 .. m) gathered into a dense padded blob with m + 1 offsets from 0, so that a
// skipped record's bytes are never examined, and validated as umis_upload validates: *bad_record is kNoRecord or the
// smallest input index of a survivor whose UMI holds a 0 byte; an empty UMI is legal.  parse_survivor_names' sibling.
int umis_gather_survivors(const uint8_t *d_umis, const uint64_t *d_umi_off, const uint32_t *d_order, uint64_t m, DevBuf<uint8_t> *d_dense,
                          DevBuf<uint64_t> *d_dense_off, uint64_t *dense_bytes, uint64_t *bad_record);
// The duplicates of a batch of nc cells whose collation is on the device: d_order (positions -> input indices, or ->
// positions of d_order_bc where that is not NULL), d_group_off (ng + 1, from 0), d_cell_group_off (nc + 1, from 0).
// cell_dups: host, nc.  With out->n_dups == 0 nothing else needs to be done.  Leaves the device idle.  Under a rule:
// cell_corrected (host, nc, or NULL) are the cells' corrected groups, and the head of a group that takes part whose
// ref_id is not below n_txps is OEM_ERR_ARG naming the smallest such input index of the batch.
int dedup_mark(const UmiInput &in, const uint32_t *d_order, const uint32_t *d_order_bc, const uint64_t *d_group_off, uint64_t ng,
               const uint64_t *d_cell_group_off, uint32_t nc, uint64_t survivor_base, UmiMarks *out, uint64_t *cell_dups,
               uint64_t *cell_corrected = nullptr);
// What the corrections since the last reset found, process-wide (the groups of the one call run on worker threads; 8
// doubles, each the sum or the maximum over the batches that ran dedup_mark with correct): [0] participants,
// [1] classes, [2] classes with a parent, [3] rounds of pointer jumping (max), [4] / [5] the longest neighbour walk in
// the first / second collation (max), [6] batches that ran the correction.
void dedup_rule_last_call(double *out8);
void dedup_rule_reset_last();
// The deduplicated collation in place of cr's arrays (m positions, nc cells; mk.n_dups > 0): *n_positions of order' are
// filled, cell_pos_off (host, nc + 1) are the cells' first positions in it.
int dedup_compact(const UmiMarks &mk, uint64_t m, uint32_t nc, CollateResident *cr, uint64_t *n_positions, uint64_t *cell_pos_off);

uint64_t collate_chunk_bytes();   // the upload chunk (testing build: OEM_COLLATE_CHUNK_BYTES)
uint64_t collate_batch_records(); // records per batch of oem_collate_names (testing build: OEM_COLLATE_BATCH_RECORDS)
constexpr uint64_t kCollateMaxBatch = (1ull << 31) - 2; // a single cell beyond this is refused (the scans take m + 1 items as an int)

// The argument checks of oem_collate_names on the input side, before any device use.
int check_collate_input(const char *who, const uint8_t *names, const uint64_t *name_off, uint64_t n_records, const uint64_t *cell_rec_off,
                        uint32_t n_cells, uint32_t mode);

} // namespace oem
