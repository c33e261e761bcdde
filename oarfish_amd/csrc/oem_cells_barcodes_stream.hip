// oem_cells_barcodes_stream.hip -- the barcoded form of the per-cell session (oem_cells_stream_set_barcodes,
// oem_cells_stream_push_barcodes): single_cell.rs:196-227 with alignment_parser.rs:244-299 from the parsed records on.
// Batches of records go up as a reader produces them, with their barcodes, read names and secondary flags, cut at ANY
// record position; the device skips the unmapped records, cuts the cells where the barcode changes, carries the open
// cell from batch to batch, and the session's group workers collate, gather, filter and run the closed cells in groups
// while later batches arrive.  The rule is stated once, in oem_collate.h ("Cells from a barcode-collated stream").
//
//   push      checks the batch on the calling thread and hands it to the staging queue (oem_stage_queue.h: the wait for
//             room in the budget -- max_staged_nnz, counted in records --, the ticket, the page-locked staging and the
//             copy outside the lock).  The session's own: the order of its refusals (the parse worker's error, the owning
//             session's sticky status, "finished"), ticket_base, and the layout the copy fills (Batch's accessors).
//   parse     the queue's one worker, batches in ticket order (process), on the null stream:
//               upload; parse_survivors drops the unmapped records; parse_survivor_names gathers the survivors' names
//               (with their flags) and barcodes into dense blobs and validates them, so that a skipped record's bytes
//               are never examined;
//               k_barcode_heads: one survivor per lane, a head when its barcode differs from the previous survivor's --
//               lengths first, then 8 bytes at a time over the padded blob; survivor 0 compares against the carried
//               open cell's barcode, which stays on the device;
//               a scan of the heads gives the batch's cell starts (k_barcode_starts); the labels of the cells it opens
//               are gathered (gather_names), one barcode per cell, and come down;
//               the survivors' records, names, flags and session-global indices are appended to the CELL ARENA, the
//               device buffer of the cells that are not yet run (a SurvivorArena, oem_dev_blob.h: its layout, growth
//               and padding are stated there, once); the batch's own buffers are released
//   the cut   once the arena's closed cells reach group_nnz records or group_cells cells (and always within the
//             driver's own group rule and a collation batch) they go to the session's group workers as groups that
//             share the arena; what is left -- closed cells short of a group and the open cell -- moves to the head of a
//             fresh arena with device-to-device copies (take_tail), so that parsing goes on under the groups' EM.  An
//             arena grows in place when its cells outgrow it: no group holds the arena the parser appends to.
//   a group   run_names_group's sequence on arena memory instead of caller memory: collate_resident in its device form
//             over the arena's names and flags, k_order_compose64 (the group's order as session-global indices, kept for
//             oem_cells_stream_barcodes_copy), records_gather, filter_device_resident, the coverage model if asked,
//             run_cells_group.  A group whose filter must take the host loop takes it (records_group_host).
//   finish    the staged batches are parsed, the open cell closes, the rest of the arena is run; the groups' pieces --
//             order, group_off, cell_group_off, kept -- and the labels are joined on the host.
//
// The ANY-ORDER form (oem_cells_stream_set_barcodes_any_order; oem_collate.h, "Cells from a stream in any order") shares
// push, staging, parse worker, arena and groups.  Its batches are not cut: their survivors' barcodes are interned
// (BarcodeIntern, oem_cells_barcodes_sort_stream.hip) and the arena keeps a cell id per survivor; nothing is handed to the
// workers before finish, which sorts the survivors by cell id, lays the arena out in that order (finish_any_order) and
// then makes the last cut of a collated arena whose cells are all closed.
//
// A UMI SESSION (oem_cells_stream_set_umis, oem_cells_stream_push_barcodes_umis; oem_collate.h, "UMIs in the sessions") is
// either form with one UMI per record.  The UMIs take the names' road: staged page-locked with the batch, uploaded, the
// survivors' gathered into a dense blob and checked for 0 bytes with the empty UMI legal (umis_gather_survivors,
// oem_dedup_umis.hip), appended to the arena's second blob (umis), carried by its growth, by the tail's move behind a
// cut and by finish_any_order's layout by cell.  A group runs dedup_mark behind collate_resident -- the arena's blob,
// its window of the UMIs' offsets indexed by group-local record -- and dedup_compact where it found duplicates;
// from there on the group has mp <= m positions, and the order, the gather (under the adjacent cut too: the order is
// no longer the identity), the filter and the host loop run over the deduplicated collation.  The slot keeps
// n_positions, the cells' first positions and cell_dups for barcodes_stream_assemble: every later group's place in
// `order` depends on what the earlier ones lost.  A session without UMIs allocates and launches nothing of this.
//
// A WHITELIST SESSION (oem_cells_stream_set_whitelist; oem_barcode_correct.h, "The rule in a session") is the any-order
// form on RAW barcodes.  Its batches run the barcodes FIRST: the mapped records' barcodes are gathered dense and checked
// (an empty one is legal), whitelist_batch (oem_barcode_correct.hip) runs the exact pass against the session's resident
// whitelist and n(w) and the neighbour pass that decides or defers, and the survivor list is compacted to the RETAINED
// records; names, UMIs, the ref_id check and the arena's append see these only.  The arena's id column holds whitelist
// ids; a deferred record's barcode and arena position go to the pending list (a DevBlob and positions).  finish decides
// the pending records with the complete counts (whitelist_finish), numbers the cells from the ids
// (barcode_cells_from_ids: correct_barcodes_resident's tail) and lays the arena out over the accepted records only.
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "oem_barcode_correct.h"
#include "oem_cells_barcodes_stream.h"
#include "oem_collate_device.h"
#include "oem_parse_device.h"
#include "oem_stage_queue.h"

namespace oem {
namespace {

constexpr int kBT = 256;
constexpr int kMaxGroupsInFlight = 3;        // groups handed to the two workers and not yet done: the parser waits beyond
constexpr uint64_t kFirstArenaRecords = 1ull << 12; // an arena starts small and doubles up to what its cells need
constexpr uint64_t kFirstArenaBytes = 64ull << 10;
constexpr int kPoolBatches = 8;              // idle staging allocations kept for reuse

inline dim3 grid_of(uint64_t n) { return dim3((unsigned)std::max<uint64_t>((n + kBT - 1) / kBT, 1)); }

// len bytes at a and at b, 8 at a time; both blobs are readable 15 bytes past their last name
__device__ __forceinline__ bool bytes_equal(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint64_t len)
{
    for (uint64_t at = 0; at < len; at += 8) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + at, 8);
        __builtin_memcpy(&y, b + at, 8);
        uint64_t d = x ^ y;
        const uint64_t left = len - at;
        if (left < 8) d &= (1ull << (8 * left)) - 1;
        if (d) return false;
    }
    return true;
}

// head[k] = survivor k starts a cell: its barcode differs from survivor k - 1's, survivor 0's from the carry's (no
// carry: a head).  off: m + 1 offsets from 0 into the dense blob bc.  head[m] = 0, for the scan over m + 1 entries.
__global__ __launch_bounds__(kBT) void k_barcode_heads(uint64_t m, const uint8_t *__restrict__ bc, const uint64_t *__restrict__ off,
                                                        const uint8_t *__restrict__ carry, uint64_t carry_len, uint32_t has_carry,
                                                        uint32_t *__restrict__ head)
{
    const uint64_t k = (uint64_t)blockIdx.x * kBT + threadIdx.x;
    if (k > m) return;
    if (k == m) {
        head[m] = 0u;
        return;
    }
    const uint64_t b0 = off[k], len = off[k + 1] - b0;
    bool h;
    if (k == 0) {
        h = !has_carry || len != carry_len || !bytes_equal(bc + b0, carry, len);
    } else {
        const uint64_t p0 = off[k - 1];
        h = b0 - p0 != len || !bytes_equal(bc + b0, bc + p0, len);
    }
    head[k] = h ? 1u : 0u;
}

// at: the exclusive scan of head.  The j-th head's survivor.
__global__ __launch_bounds__(kBT) void k_barcode_starts(uint64_t m, const uint32_t *__restrict__ head, const uint64_t *__restrict__ at,
                                                         uint32_t *__restrict__ start)
{
    const uint64_t k = (uint64_t)blockIdx.x * kBT + threadIdx.x;
    if (k < m && head[k]) start[at[k]] = (uint32_t)k;
}

// out[k] = gidx[order[k]]: a group's collated positions as session-global indices (k_order_compose over 64 bits)
__global__ __launch_bounds__(kBT) void k_order_compose64(uint64_t m, const uint32_t *__restrict__ order, const uint64_t *__restrict__ gidx,
                                                          uint64_t *__restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * kBT + threadIdx.x;
    if (k < m) out[k] = gidx[order[k]];
}

inline size_t up64(size_t v) { return (v + 63) & ~(size_t)63; }

// A staged batch: the records, the two offset tables, the flags, the two blobs; in a UMI session the UMIs' offset table
// and blob behind them.
struct Batch : StageBatch {
    uint64_t bc_bytes = 0, name_bytes = 0, umi_bytes = 0;
    bool has_sec = false, has_umis = false;
    size_t at_bc_off() const { return up64(sizeof(oem_aln_record) * n_records); }
    size_t at_name_off() const { return at_bc_off() + up64(sizeof(uint64_t) * (n_records + 1)); }
    size_t at_sec() const { return at_name_off() + up64(sizeof(uint64_t) * (n_records + 1)); }
    size_t at_bc() const { return at_sec() + up64(n_records); }
    size_t at_names() const { return at_bc() + up64(bc_bytes); }
    size_t at_umi_off() const { return at_names() + up64(name_bytes); }
    size_t at_umis() const { return at_umi_off() + up64(sizeof(uint64_t) * (n_records + 1)); }
    size_t bytes() const { return has_umis ? at_umis() + up64(umi_bytes) : at_umi_off(); }
    const char *base() const { return (const char *)mem.p; }
};

// What a group leaves for oem_cells_stream_barcodes_copy, from 0.
struct Slot {
    uint32_t n_cells = 0;
    uint64_t n_records = 0, n_groups = 0;
    std::vector<uint64_t> order, group_off, cell_group_off; // n_positions; n_groups + 1; n_cells + 1
    std::vector<uint32_t> kept;                             // n_groups
    // n_records positions, or in a UMI session those that remain: then group_off and cell_group_off are the deduplicated
    // collation's, with the cells' first positions in it and the duplicates (reads) that every cell lost
    uint64_t n_positions = 0;
    std::vector<uint64_t> cell_pos_off, cell_dups;          // n_cells + 1; n_cells (a UMI session)
    std::vector<uint64_t> cell_corrected;                   // n_cells (a UMI session under a rule with correct)
    bool done = false;
};

struct U32AsU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

} // namespace

int exclusive_scan_u32(const uint32_t *d_in, uint64_t *d_out, uint64_t n)
{
    hipcub::TransformInputIterator<uint64_t, U32AsU64, const uint32_t *> in(d_in, U32AsU64());
    size_t tb = 0;
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, d_out, (int)n, nullptr));
    DevBuf<uint8_t> tmp;
    OEM_TRY(dev_alloc(&tmp.p, tb, nullptr));
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, in, d_out, (int)n, nullptr));
    OEM_HIP(hipStreamSynchronize(nullptr));
    return OEM_OK;
}

struct BarcodesStream {
    BarcodesEnv env;

    // The staging queue of the batches (oem_stage_queue.h) with the parse worker.  Its lock is this part's own lock too.
    StageQueue<Batch> q;
    std::mutex &mu = q.mu;
    std::condition_variable cv_groups;        // the group hand-off of cut_groups: not the queue's
    std::vector<uint64_t> ticket_base;        // by ticket: the session-global index of the batch's first record
    int groups_in_flight = 0;
    bool closed = false, cancel = false;
    int stuck_rc = OEM_OK; // the parse worker's own error (the session's sticky status holds it too)
    std::string stuck_msg;

    // -- the parse worker's state (no lock: one thread; finish reads it after the join) ---------------------------------
    // The cells that are not yet run (SurvivorArena, oem_dev_blob.h; with the survivors' cell ids in an any-order
    // session, their UMIs in a UMI session).  It grows in place under the appends, which is sound because THE PARSE
    // WORKER NEVER APPENDS TO AN ARENA THAT A GROUP HOLDS: cut_groups moves the arena out of this member before the
    // first group of a call captures it, so on every return -- the cancelled wait and the errors included -- `arena`
    // is a fresh one with the tail, or none.  A cancelled part drops arena and cells, and parses no further batch.
    std::shared_ptr<SurvivorArena> arena;
    std::vector<uint64_t> cstart;              // the arena's cells: their first survivors; the last one is open
    uint64_t first_cell = 0;                   // the session's number of the arena's first cell
    DevBuf<uint8_t> carry;                     // the open cell's barcode, padded by 16
    uint64_t carry_len = 0;
    uint64_t n_unmapped = 0, n_survivors = 0, run_records = 0; // run_records: survivors handed to the workers
    std::vector<uint8_t> labels;               // every opened cell's barcode, in cell order
    std::vector<uint64_t> label_off{0};
    std::deque<std::unique_ptr<Slot>> slots;   // by group (mu: the deque itself; a slot is its group's alone)
    // an any-order session (oem_cells_barcodes_sort_stream.hip): the table of the labels seen so far; the arena keeps a
    // cell id per survivor and nothing is cut before finish
    bool any_order = false;
    BarcodeIntern intern;
    // a UMI session (oem_cells_stream_set_umis; oem_collate.h, "UMIs in the sessions"): every batch brings a UMI per
    // record, the arena keeps the survivors', and a group is deduplicated behind its name collation
    bool with_umis = false;
    uint64_t dup_reads = 0, dup_records = 0;   // (mu) of the groups that have run
    std::vector<uint64_t> out_cell_dups;
    // the UMI rule (oem_cells_stream_set_umi_rule; oem_collate.h, "The UMI rule"): set once before the first push; the
    // group workers only read it.  gene_of is the session's copy, d_gene_of its upload to the session's device.
    bool rule_set = false;
    std::vector<uint32_t> gene_of;
    DevBuf<uint32_t> d_gene_of;
    uint32_t rule_correct = 0;
    uint64_t corrected_reads = 0;              // (mu) of the groups that have run
    std::vector<uint64_t> out_cell_corrected;
    uint64_t arena_peak = 0, info_misses = 0, info_slots = 0; // (mu) as of the last batch, for oem_cells_stream_info
    // a whitelist session (oem_cells_stream_set_whitelist; oem_barcode_correct.h, "The rule in a session"): the resident
    // whitelist with the session's n(w), built when the rule is set, and the session's copy of its labels; the pending
    // list of the deferred records -- their barcodes and arena positions, in arena order --, grown as the arena grows
    std::unique_ptr<BarcodeWhitelist> wl; // (released at finish and on an error)
    bool wl_was_set = false;
    std::vector<uint8_t> wl_labels;
    std::vector<uint64_t> wl_label_off;
    DevBlob pending;
    DevBuf<uint32_t> pending_pos;
    uint64_t pending_pos_cap = 0;
    uint64_t wl_counts[kBarcodeStatuses] = {0, 0, 0, 0, 0}, wl_rejected = 0, wl_deferred = 0; // (mu)
    std::vector<uint32_t> out_cell_wl_id;
    std::vector<uint64_t> out_cell_bc_corrected;

    // -- what finish leaves ------------------------------------------------------------------------------------------------
    bool assembled = false;
    std::vector<uint64_t> out_cell_rec_off, out_order, out_group_off, out_cell_group_off;
    std::vector<uint32_t> out_kept;

    explicit BarcodesStream(const BarcodesEnv &e)
        : env(e), q(e.max_staged, kPoolBatches,
                    [this](size_t bytes, StageMem *m) {
                        if (stage_host_alloc(env.device, bytes, m)) return true;
                        set_stuck(OEM_ERR_OOM, "oem_cells_stream_push_barcodes: host allocation of the staging memory failed");
                        return false;
                    },
                    stage_host_free)
    {
    }
    uint64_t n_cells_opened() const { return label_off.size() - 1; }
    void set_stuck(int rc, const char *msg)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (stuck_rc == OEM_OK) {
                stuck_rc = rc;
                stuck_msg = msg;
            }
        }
        env.set_sticky(rc, msg);
        q.wake_pushers();
    }
    uint64_t ticket_of(uint64_t record)
    {
        std::lock_guard<std::mutex> lk(mu);
        return (uint64_t)(std::upper_bound(ticket_base.begin(), ticket_base.end(), record) - ticket_base.begin()) - 1;
    }

    void note_arena_bytes(uint64_t held)
    {
        std::lock_guard<std::mutex> lk(mu);
        arena_peak = std::max(arena_peak, held);
    }
    std::shared_ptr<SurvivorArena> new_arena(bool with_ids) const // (empty: nothing is allocated yet)
    {
        return std::make_shared<SurvivorArena>(kFirstArenaRecords, kFirstArenaBytes, with_ids, with_umis);
    }
    int intern_batch(const Batch &b, const char *who, const oem_aln_record *d_in, const uint32_t *d_order, uint64_t m, const uint8_t *d_dbc,
                     const uint64_t *d_dbc_off, DevBuf<uint32_t> *d_cell_id);
    int whitelist_barcodes(const Batch &b, const char *who, const uint8_t *d_bc, const uint64_t *d_bc_off, const uint32_t *d_order, uint64_t m,
                           WhitelistBatch *wb);
    int whitelist_retain(const Batch &b, const char *who, const oem_aln_record *d_in, const uint32_t *d_retained, const WhitelistBatch &wb);
    int whitelist_cells(const char *who, BarcodeCells *bc, uint64_t *n_accepted);
    void release_whitelist()
    {
        wl.reset();
        pending.release();
        pending_pos.reset();
        pending_pos_cap = 0;
    }
    uint64_t pending_held() const { return pending.held() + sizeof(uint32_t) * pending_pos_cap; }
    int finish_any_order(const char *who);
    int run_batch(const Batch &b);
    int cut_groups(bool final);
    int run_group(const std::shared_ptr<SurvivorArena> &a, const std::vector<uint64_t> &cro, uint64_t cell0, Slot *slot, StreamGroupResult *out,
                  bool *batched);
    void process(Batch &b, bool skip);
};

// An any-order session's batch behind its name checks: the ref_ids while the batch still knows its ticket, the bound on
// the survivors (finish collates them as one batch), then the cells of the m survivors from the table.
int BarcodesStream::intern_batch(const Batch &b, const char *who, const oem_aln_record *d_in, const uint32_t *d_order, uint64_t m,
                                 const uint8_t *d_dbc, const uint64_t *d_dbc_off, DevBuf<uint32_t> *d_cell_id)
{
    uint64_t bad = kNoRecord;
    OEM_TRY(records_ref_check(m, d_order, d_in, env.n_txps, &bad));
    if (bad != kNoRecord) {
        const oem_aln_record *h = (const oem_aln_record *)b.base();
        return fail(OEM_ERR_ARG, "%s: record %llu: ref_id %u is not below n_txps", who, (unsigned long long)(b.rec_base + bad), h[bad].ref_id);
    }
    if ((arena ? arena->n : 0) + m > kCollateMaxBatch)
        return fail(OEM_ERR_ARG, "%s: more than 2^31 - 2 surviving records in the session: its cells are found by one sort at finish", who);
    OEM_TRY(dev_alloc(&d_cell_id->p, m, nullptr));
    OEM_TRY(intern.batch(who, d_dbc, d_dbc_off, m, d_cell_id->p));
    std::lock_guard<std::mutex> lk(mu);
    info_misses = intern.misses;
    info_slots = intern.capacity;
    return OEM_OK;
}

// A whitelist session's batch, first step: the m mapped records' barcodes gathered dense -- an unmapped record's are never
// examined, an empty one is legal, a 0 byte is the batch's error --, then the rule's two passes and the compaction to the
// retained records (whitelist_batch).
int BarcodesStream::whitelist_barcodes(const Batch &b, const char *who, const uint8_t *d_bc, const uint64_t *d_bc_off, const uint32_t *d_order,
                                       uint64_t m, WhitelistBatch *wb)
{
    DevBuf<uint8_t> d_dbc;
    DevBuf<uint64_t> d_dbc_off;
    uint64_t dbc_bytes = 0, bad = kNoRecord;
    OEM_TRY(umis_gather_survivors(d_bc, d_bc_off, d_order, m, &d_dbc, &d_dbc_off, &dbc_bytes, &bad));
    if (bad != kNoRecord)
        return fail(OEM_ERR_ARG, "%s: the barcode of record %llu contains a 0 byte", who, (unsigned long long)(b.rec_base + bad));
    OEM_TRY(whitelist_batch(who, *wl, d_dbc.p, d_dbc_off.p, d_order, m, arena ? arena->n : 0, wb));
    std::lock_guard<std::mutex> lk(mu);
    for (int k = 0; k < kBarcodeStatuses; ++k) wl_counts[k] += wb->counts[k];
    wl_rejected += wb->counts[kBarcodeNoNeighbour] + wb->counts[kBarcodeAmbiguous] + wb->counts[kBarcodeMissing];
    wl_deferred += wb->n_deferred;
    return OEM_OK;
}

// ... and behind the name and UMI checks of the retained records: their ref_ids while the batch still knows its ticket,
// the bound on the retained records, and the deferred ones onto the pending list.
int BarcodesStream::whitelist_retain(const Batch &b, const char *who, const oem_aln_record *d_in, const uint32_t *d_retained,
                                     const WhitelistBatch &wb)
{
    uint64_t bad = kNoRecord;
    OEM_TRY(records_ref_check(wb.n_retained, d_retained, d_in, env.n_txps, &bad));
    if (bad != kNoRecord) {
        const oem_aln_record *h = (const oem_aln_record *)b.base();
        return fail(OEM_ERR_ARG, "%s: record %llu: ref_id %u is not below n_txps", who, (unsigned long long)(b.rec_base + bad), h[bad].ref_id);
    }
    if ((arena ? arena->n : 0) + wb.n_retained > kCollateMaxBatch)
        return fail(OEM_ERR_ARG, "%s: more than 2^31 - 2 retained records in the session: its cells are found by one sort at finish", who);
    if (wb.n_deferred == 0) return OEM_OK;
    OEM_TRY(pending.reserve(pending.n + wb.n_deferred, pending.n_bytes + wb.deferred_bytes, 1024, 4096, 0, nullptr));
    if (pending.cap > pending_pos_cap) { // the positions grow with the blob's entries
        DevBuf<uint32_t> grown;
        OEM_TRY(dev_alloc(&grown.p, pending.cap, nullptr));
        if (pending.n) OEM_HIP(hipMemcpy(grown.p, pending_pos.p, sizeof(uint32_t) * pending.n, hipMemcpyDeviceToDevice));
        std::swap(pending_pos.p, grown.p);
        pending_pos_cap = pending.cap;
    }
    OEM_HIP(hipMemcpy(pending_pos.p + pending.n, wb.deferred_pos.p, sizeof(uint32_t) * wb.n_deferred, hipMemcpyDeviceToDevice));
    OEM_TRY(pending.append(wb.deferred_bc.p, wb.deferred_off.p, wb.n_deferred, wb.deferred_bytes));
    OEM_HIP(hipStreamSynchronize(nullptr));
    return OEM_OK;
}

// A whitelist session's finish: the pending records decided with the complete counts, the cells from the arena's ids,
// every cell's whitelist id and corrected records, and the labels -- the whitelist's bytes -- from the session's copy.
int BarcodesStream::whitelist_cells(const char *who, BarcodeCells *bc, uint64_t *n_accepted)
{
    const uint64_t m = arena->n;
    uint64_t late[kBarcodeStatuses];
    OEM_TRY(whitelist_finish(who, *wl, pending.bytes.p, pending.off.p, pending_pos.p, pending.n, arena->cell_id.p, m, late));
    if (late[kBarcodeCorrected] + late[kBarcodeAmbiguous] != pending.n)
        return fail(OEM_ERR_STATE, "%s: %llu pending records, %llu of them decided", who, (unsigned long long)pending.n,
                    (unsigned long long)(late[kBarcodeCorrected] + late[kBarcodeAmbiguous]));
    {
        std::lock_guard<std::mutex> lk(mu);
        for (int k = 0; k < kBarcodeStatuses; ++k) wl_counts[k] += late[k];
        wl_rejected += late[kBarcodeAmbiguous];
    }
    OEM_TRY(barcode_cells_from_ids(who, arena->cell_id.p, ~kBarcodeCorrectedBit, m, wl->n_labels, m - late[kBarcodeAmbiguous], bc, n_accepted));
    OEM_TRY(whitelist_cell_summary(*bc, arena->cell_id.p, &out_cell_wl_id, &out_cell_bc_corrected));
    labels.clear();
    label_off.assign(1, 0);
    for (const uint32_t w : out_cell_wl_id) {
        if (w >= wl->n_labels) return fail(OEM_ERR_STATE, "%s: a cell has the whitelist id %u of %llu", who, w, (unsigned long long)wl->n_labels);
        labels.insert(labels.end(), wl_labels.begin() + wl_label_off[w], wl_labels.begin() + wl_label_off[w + 1]);
        label_off.push_back(labels.size());
    }
    return OEM_OK;
}

// An any-order session's finish, after the parse worker's end and before the last cut: the survivors sorted by cell id,
// the arena laid out in that order -- from here on it is a collated session's arena whose cells are all closed -- and
// the labels down.
int BarcodesStream::finish_any_order(const char *who)
{
    intern.publish_last();
    uint64_t m = arena ? arena->n : 0;
    if (m == 0) {
        intern.release();
        release_whitelist();
        return OEM_OK;
    }
    BarcodeCells bc;
    const uint64_t n_arena = m; // a whitelist session: the retained records; m becomes the accepted ones, which are laid out
    if (wl) {
        OEM_TRY(whitelist_cells(who, &bc, &m));
        release_whitelist();
        n_survivors = m;
        if (m == 0) { // every retained record was rejected at last: no cells
            arena.reset();
            return OEM_OK;
        }
    } else {
        OEM_TRY(intern.cells(arena->cell_id.p, m, &bc));
        OEM_TRY(intern.labels_down(&labels, &label_off));
    }
    intern.release();
    const uint64_t nc = bc.n_cells;
    const SurvivorArena &a = *arena;
    std::shared_ptr<SurvivorArena> na = new_arena(false); // at exact size: nothing is appended to it
    OEM_TRY(na->make(m, a.names.n_bytes, a.umis.n_bytes));
    note_arena_bytes(a.held() + na->held());
    // the gathers write whole words, which leaves fewer zeros than the arena's invariant asks: the memsets complete them
    auto gather_blob = [&](const DevBlob &src, DevBlob &dst, const uint8_t *src_sec, uint8_t *dst_sec, bool with_empty) {
        OEM_TRY(gather_name_offsets(bc.order.p, m, src.off.p, dst.off.p));
        uint64_t n_bytes = src.n_bytes; // (of the accepted records only where some were rejected at finish)
        if (m != n_arena) OEM_HIP(hipMemcpy(&n_bytes, dst.off.p + m, sizeof n_bytes, hipMemcpyDeviceToHost));
        OEM_TRY(gather_names(bc.order.p, m, src.bytes.p, src.off.p, dst.off.p, 0, n_bytes, dst.bytes.p, src_sec, dst_sec, with_empty));
        OEM_HIP(hipMemsetAsync(dst.bytes.p + n_bytes, 0, kBlobPad, nullptr));
        dst.n = m;
        dst.n_bytes = n_bytes;
        return (int)OEM_OK;
    };
    OEM_TRY(records_gather(m, bc.order.p, a.rec.p, na->rec.p));
    OEM_TRY(gather_blob(a.names, na->names, a.sec.p, na->sec.p, false));
    if (with_umis) OEM_TRY(gather_blob(a.umis, na->umis, nullptr, nullptr, true)); // in cell order, as the names
    OEM_HIP(hipMemsetAsync(na->sec.p + m, 0, kFlagPad, nullptr));
    hipLaunchKernelGGL(k_order_compose64, grid_of(m), dim3(kBT), 0, nullptr, m, (const uint32_t *)bc.order.p, (const uint64_t *)a.gidx.p,
                       na->gidx.p);
    OEM_HIP(hipGetLastError());
    na->n = m;
    cstart.assign(nc, 0); // the cells: their first survivors
    OEM_HIP(hipMemcpy(cstart.data(), bc.cell_rec_off.p, sizeof(uint64_t) * nc, hipMemcpyDeviceToHost));
    first_cell = 0;
    arena = std::move(na);
    (void)who;
    return OEM_OK;
}

// One batch on the parse worker: see the head of the file.
int BarcodesStream::run_batch(const Batch &b)
{
    const uint64_t n = b.n_records;
    if (n == 0) return OEM_OK;
    char who[64];
    snprintf(who, sizeof who, "oem_cells_stream: ticket %llu", (unsigned long long)b.ticket);
    DevBuf<oem_aln_record> d_in;
    DevBuf<uint8_t> d_bc, d_names, d_sec;
    DevBuf<uint64_t> d_bc_off, d_name_off;
    OEM_TRY(dev_alloc(&d_in.p, n, nullptr));
    OEM_HIP(hipMemcpyAsync(d_in.p, b.base(), sizeof(oem_aln_record) * n, hipMemcpyHostToDevice, nullptr));
    auto up = [&](size_t at_bytes, uint64_t n_bytes, size_t at_off, DevBuf<uint8_t> *d_bytes, DevBuf<uint64_t> *d_off) {
        return upload_blob_async((const uint8_t *)b.base() + at_bytes, n_bytes, (const uint64_t *)(b.base() + at_off), n, 0, 0, d_bytes, d_off);
    };
    OEM_TRY(up(b.at_bc(), b.bc_bytes, b.at_bc_off(), &d_bc, &d_bc_off));
    OEM_TRY(up(b.at_names(), b.name_bytes, b.at_name_off(), &d_names, &d_name_off));
    if (b.has_sec) OEM_TRY(upload_flags_async((const uint8_t *)b.base() + b.at_sec(), n, &d_sec));
    DevBuf<uint8_t> d_umis;
    DevBuf<uint64_t> d_umi_off;
    if (with_umis) OEM_TRY(up(b.at_umis(), b.umi_bytes, b.at_umi_off(), &d_umis, &d_umi_off)); // (a UMI session's batch always has its offsets)
    OEM_HIP(hipStreamSynchronize(nullptr));

    // the survivors; their barcodes and names as dense blobs, checked
    DevBuf<uint32_t> d_order;
    uint64_t m = 0;
    OEM_TRY(parse_survivors(d_in.p, n, true, &d_order, &m));
    n_unmapped += n - m;
    if (m == 0) return OEM_OK;
    // a whitelist session: the barcodes first; from here on the batch's survivors are its retained records
    WhitelistBatch wb;
    if (wl) {
        OEM_TRY(whitelist_barcodes(b, who, d_bc.p, d_bc_off.p, d_order.p, m, &wb));
        if (wb.n_retained == 0) return OEM_OK; // (every mapped record was rejected: nothing else of the batch is looked at)
        std::swap(d_order.p, wb.order.p); // (wb.order: the mapped records from here on; released with wb)
        m = wb.n_retained;
    }
    DevBuf<uint8_t> d_dbc, d_dnames, d_dsec, d_none;
    DevBuf<uint64_t> d_dbc_off, d_dname_off;
    uint64_t dbc_bytes = 0, dname_bytes = 0, bad_bc = kNoRecord, bad_name = kNoRecord;
    bool zero_bc = false, zero_name = false;
    if (!wl)
        OEM_TRY(parse_survivor_names(d_bc.p, b.bc_bytes, d_bc_off.p, n, d_order.p, m, nullptr, &d_dbc, &d_dbc_off, &d_none, &dbc_bytes, &bad_bc,
                                     &zero_bc));
    OEM_TRY(parse_survivor_names(d_names.p, b.name_bytes, d_name_off.p, n, d_order.p, m, d_sec.p, &d_dnames, &d_dname_off, &d_dsec,
                                 &dname_bytes, &bad_name, &zero_name));
    // a UMI session: the survivors' UMIs likewise, an empty one being legal.  On one record the barcode's error comes
    // first, then the name's, then the UMI's.
    DevBuf<uint8_t> d_dumis;
    DevBuf<uint64_t> d_dumi_off;
    uint64_t dumi_bytes = 0, bad_umi = kNoRecord;
    if (with_umis) OEM_TRY(umis_gather_survivors(d_umis.p, d_umi_off.p, d_order.p, m, &d_dumis, &d_dumi_off, &dumi_bytes, &bad_umi));
    if (bad_umi != kNoRecord && bad_umi < bad_bc && bad_umi < bad_name)
        return fail(OEM_ERR_ARG, "%s: the UMI of record %llu contains a 0 byte", who, (unsigned long long)(b.rec_base + bad_umi));
    d_umis.reset();
    d_umi_off.reset();
    if (bad_bc != kNoRecord && bad_bc <= bad_name) {
        if (zero_bc)
            return fail(OEM_ERR_ARG, "%s: the barcode of record %llu contains a 0 byte", who, (unsigned long long)(b.rec_base + bad_bc));
        return fail(OEM_ERR_ARG, "%s: record %llu has an empty barcode", who, (unsigned long long)(b.rec_base + bad_bc));
    }
    if (bad_name != kNoRecord) return parse_bad_name(who, zero_name, b.rec_base + bad_name);
    d_bc.reset();
    d_bc_off.reset();
    d_names.reset();
    d_name_off.reset();

    // the batch's survivors into the arena, which the first of them makes
    auto append = [&](const uint32_t *d_cell_id) {
        if (!arena) arena = new_arena(any_order);
        OEM_TRY(arena->append(m, d_order.p, d_in.p, n, b.rec_base, d_dnames.p, d_dname_off.p, dname_bytes, d_dsec.p, d_cell_id, d_dumis.p,
                              d_dumi_off.p, dumi_bytes));
        note_arena_bytes(arena->peak);
        n_survivors += m;
        return (int)OEM_OK;
    };
    if (wl) { // the retained records with their whitelist ids; the deferred ones onto the pending list
        OEM_TRY(whitelist_retain(b, who, d_in.p, d_order.p, wb));
        OEM_TRY(append(wb.id.p));
        note_arena_bytes(arena->peak + pending_held());
        return OEM_OK;
    }
    if (any_order) { // the survivors' cells from the table; the arena takes them with their cell ids, and nothing is cut
        DevBuf<uint32_t> d_cell_id;
        OEM_TRY(intern_batch(b, who, d_in.p, d_order.p, m, d_dbc.p, d_dbc_off.p, &d_cell_id));
        d_dbc.reset();
        d_dbc_off.reset();
        return append(d_cell_id.p);
    }

    // the heads and the batch's cell starts
    DevBuf<uint32_t> d_head, d_start;
    DevBuf<uint64_t> d_at;
    OEM_TRY(dev_alloc(&d_head.p, m + 1, nullptr));
    OEM_TRY(dev_alloc(&d_at.p, m + 1, nullptr));
    const bool has_carry = !cstart.empty();
    hipLaunchKernelGGL(k_barcode_heads, grid_of(m + 1), dim3(kBT), 0, nullptr, m, (const uint8_t *)d_dbc.p, (const uint64_t *)d_dbc_off.p,
                       (const uint8_t *)carry.p, carry_len, has_carry ? 1u : 0u, d_head.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(exclusive_scan_u32(d_head.p, d_at.p, m + 1));
    uint64_t nh = 0;
    OEM_HIP(hipMemcpy(&nh, d_at.p + m, sizeof nh, hipMemcpyDeviceToHost));
    std::vector<uint32_t> start(nh);
    if (nh) {
        OEM_TRY(dev_alloc(&d_start.p, nh, nullptr));
        hipLaunchKernelGGL(k_barcode_starts, grid_of(m), dim3(kBT), 0, nullptr, m, (const uint32_t *)d_head.p, (const uint64_t *)d_at.p, d_start.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpy(start.data(), d_start.p, sizeof(uint32_t) * nh, hipMemcpyDeviceToHost));
        // the labels of the cells the batch opens: one barcode per cell; the last one is the new carry
        DevBuf<uint64_t> d_lab_off;
        DevBuf<uint8_t> d_lab;
        uint64_t lab_bytes = 0;
        OEM_TRY(gather_input_names(d_start.p, nh, d_dbc.p, d_dbc_off.p, &d_lab_off, &d_lab, &lab_bytes));
        std::vector<uint64_t> lab_off(nh + 1);
        OEM_HIP(hipMemcpy(lab_off.data(), d_lab_off.p, sizeof(uint64_t) * (nh + 1), hipMemcpyDeviceToHost));
        const size_t l0 = labels.size();
        labels.resize(l0 + lab_bytes);
        if (lab_bytes) OEM_HIP(hipMemcpy(labels.data() + l0, d_lab.p, lab_bytes, hipMemcpyDeviceToHost));
        label_off.reserve(label_off.size() + nh);
        for (uint64_t j = 0; j < nh; ++j) label_off.push_back(l0 + lab_off[j + 1]);
        carry_len = lab_off[nh] - lab_off[nh - 1];
        carry.reset();
        OEM_TRY(dev_alloc(&carry.p, carry_len + 16, nullptr));
        OEM_HIP(hipMemset(carry.p, 0, carry_len + 16));
        OEM_HIP(hipMemcpy(carry.p, d_lab.p + lab_off[nh - 1], carry_len, hipMemcpyDeviceToDevice));
    }
    d_head.reset();
    d_at.reset();
    d_dbc.reset();
    d_dbc_off.reset();

    const uint64_t n0 = arena ? arena->n : 0;
    OEM_TRY(append(nullptr));
    for (uint64_t j = 0; j < nh; ++j) cstart.push_back(n0 + start[j]);
    return cut_groups(false);
}

// The arena's closed cells (final: all of its cells) in groups to the workers, as far as they fill groups; the rest moves
// to the head of a fresh arena.
int BarcodesStream::cut_groups(bool final)
{
    const uint64_t arena_n = arena ? arena->n : 0;
    const size_t n_all = cstart.size(), n_closed = final ? n_all : (n_all ? n_all - 1 : 0);
    auto cell_end = [&](size_t i) { return i + 1 < n_all ? cstart[i + 1] : arena_n; };
    const uint64_t hard = cells_max_group_nnz(), max_batch = std::min<uint64_t>(collate_batch_records(), kCollateMaxBatch);
    std::shared_ptr<SurvivorArena> old; // the arena from the first hand-over on: the groups', no longer this part's
    size_t i = 0;
    while (i < n_closed) {
        size_t j = i;
        uint64_t recs = 0;
        bool full = false;
        while (j < n_closed) {
            const uint64_t sz = cell_end(j) - cstart[j];
            if (sz > kCollateMaxBatch)
                return fail(OEM_ERR_ARG, "oem_cells_stream: cell %llu has %llu records: at most 2^31 - 2 per cell",
                            (unsigned long long)(first_cell + j), (unsigned long long)sz);
            if (j > i && (!cells_group_fits((uint64_t)(j - i) + 1, recs + sz, recs + sz, env.n_txps, hard) || recs + sz > max_batch)) {
                full = true;
                break;
            }
            recs += sz;
            ++j;
            if (recs >= env.group_nnz || j - i >= env.group_cells) {
                full = true;
                break;
            }
        }
        if (!full && !final) break;
        { // the workers take a few groups at a time: every group holds its arena
            std::unique_lock<std::mutex> lk(mu);
            cv_groups.wait(lk, [&] { return groups_in_flight < kMaxGroupsInFlight || cancel; });
            if (cancel) { // (nothing more is parsed: process)
                arena.reset();
                cstart.clear();
                return OEM_OK;
            }
            ++groups_in_flight;
        }
        std::vector<uint64_t> cro(j - i + 1);
        for (size_t c = i; c < j; ++c) cro[c - i] = cstart[c];
        cro[j - i] = cell_end(j - 1);
        Slot *slot;
        {
            std::lock_guard<std::mutex> lk(mu);
            slots.emplace_back(new Slot());
            slot = slots.back().get();
        }
        slot->n_cells = (uint32_t)(j - i);
        slot->n_records = recs;
        struct InFlight { // released when the group has run, or with the group when it never does
            BarcodesStream *b;
            ~InFlight()
            {
                {
                    std::lock_guard<std::mutex> lk(b->mu);
                    --b->groups_in_flight;
                }
                b->cv_groups.notify_all();
            }
        };
        std::shared_ptr<InFlight> guard(new InFlight{this});
        if (!old) old.swap(arena); // (`arena` is none from here on)
        std::shared_ptr<SurvivorArena> a = old;
        const uint64_t cell0 = first_cell + i;
        run_records += recs;
        env.submit([this, a, cro, cell0, slot, guard](StreamGroupResult *out, bool *batched) {
            (void)guard;
            return run_group(a, cro, cell0, slot, out, batched);
        });
        i = j;
    }
    if (i == 0) return OEM_OK;
    // what is left moves to the head of a fresh arena; the groups keep the old one
    const uint64_t t = i < n_all ? cstart[i] : arena_n;
    if (!final) { // (the tail's first name and UMI bytes are the old arena's offsets at t)
        uint64_t tb = 0, tub = 0;
        OEM_HIP(hipMemcpy(&tb, old->names.off.p + t, sizeof tb, hipMemcpyDeviceToHost));
        if (with_umis) OEM_HIP(hipMemcpy(&tub, old->umis.off.p + t, sizeof tub, hipMemcpyDeviceToHost));
        const uint64_t tail_n = arena_n - t, tail_bytes = old->names.n_bytes - tb, tail_umi_bytes = old->umis.n_bytes - tub;
        const uint64_t cap = std::max(tail_n, std::min(old->cap, 2 * env.group_nnz)) + 4096;
        std::shared_ptr<SurvivorArena> fresh = new_arena(false);
        OEM_TRY(fresh->make(cap, std::max(tail_bytes, std::min<uint64_t>(old->names.cap_bytes, 64 * cap)) + 4096,
                            std::max(tail_umi_bytes, std::min<uint64_t>(old->umis.cap_bytes, 16 * cap)) + 4096));
        OEM_TRY(fresh->take_tail(*old, t, tb, tub));
        arena = std::move(fresh);
    }
    first_cell += i;
    cstart.erase(cstart.begin(), cstart.begin() + i);
    for (uint64_t &v : cstart) v -= t;
    return OEM_OK;
}

// One group on a group worker: the cells at cro[0 .. n_cells] of the arena `a`, the session's cells cell0 ...
int BarcodesStream::run_group(const std::shared_ptr<SurvivorArena> &a, const std::vector<uint64_t> &cro, uint64_t cell0, Slot *slot,
                              StreamGroupResult *out, bool *batched)
{
    *batched = false;
    const char *who = "oem_cells_stream";
    StageTimer tm;
    const uint32_t n_cells = (uint32_t)(cro.size() - 1);
    const uint64_t r0 = cro[0], m = cro[n_cells] - r0; // (m > 0: a cell holds a survivor)
    const RecordsFilter &rf = *env.rf;
    const bool keep = knob("OEM_TEST_KEEP_RECORDS_CSR", 0) != 0;
    CellsRun run{env.n_txps, env.device, env.max_iter, env.conv_thresh, env.cov};
    OEM_TRY(ensure_device(env.device));
    out->infos.assign(n_cells, oem_run_info{});
    out->tables.assign(n_cells, oem_discard_table{});

    CollateInput in;
    in.who = who;
    in.cell_rec_off = cro.data();
    in.mode = env.mode;
    in.chunk_bytes = collate_chunk_bytes();
    in.d_names = a->names.bytes.p;
    in.d_name_off = a->names.off.p + r0;
    in.d_secondary = a->sec.p + r0;
    CollateResident cr;
    double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    OEM_TRY(collate_resident(in, 0, n_cells, 0, 0, 0, info, &cr));
    tm.lap("barcodes: collate");
    auto bad_ref = [&](uint64_t record, uint32_t ref_id) { // record: the session-global index
        return fail(OEM_ERR_ARG, "%s: ticket %llu: record %llu: ref_id %u is not below n_txps", who, (unsigned long long)ticket_of(record),
                    (unsigned long long)record, ref_id);
    };
    uint64_t mp = m; // the positions of the group's order: fewer than its records once duplicates are dropped
    if (a->with_umis) { // the duplicates leave the collation here: their records are never gathered
        slot->cell_dups.assign(n_cells, 0);
        slot->cell_pos_off.assign((size_t)n_cells + 1, 0);
        UmiInput um; // the arena's UMIs; the group's window of their offsets is indexed by group-local record
        um.who = who;
        um.d_umis = a->umis.bytes.p;
        um.d_umi_off = a->umis.off.p + r0;
        if (d_gene_of.p) { // the rule's gene keys: the heads' ref_ids are word 0 of the arena's records
            um.d_ref_id = reinterpret_cast<const uint32_t *>(a->rec.p + r0);
            um.ref_id_stride = sizeof(oem_aln_record) / sizeof(uint32_t);
            um.d_gene_of = d_gene_of.p;
            um.n_txps = env.n_txps;
            um.defer_bad_ref = true;
        }
        um.correct = rule_correct;
        if (rule_correct) slot->cell_corrected.assign(n_cells, 0);
        UmiMarks mk;
        OEM_TRY(dedup_mark(um, cr.order.p, nullptr, cr.group_off.p, cr.n_groups, cr.cell_group_off.p, n_cells, 0, &mk, slot->cell_dups.data(),
                           rule_correct ? slot->cell_corrected.data() : nullptr));
        if (mk.bad_ref_record != kCollateNoRecord) { // a group-local record: the arena knows it by its session index
            uint64_t record = 0;
            OEM_HIP(hipMemcpy(&record, a->gidx.p + r0 + mk.bad_ref_record, sizeof record, hipMemcpyDeviceToHost));
            return bad_ref(record, mk.bad_ref_id);
        }
        if (mk.n_dups) {
            OEM_TRY(dedup_compact(mk, m, n_cells, &cr, &mp, slot->cell_pos_off.data()));
        } else {
            for (uint32_t c = 0; c <= n_cells; ++c) slot->cell_pos_off[c] = cro[c] - r0;
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            dup_reads += mk.n_dups;
            dup_records += m - mp;
            for (uint64_t v : slot->cell_corrected) corrected_reads += v;
        }
        tm.lap("barcodes: dedup");
    }
    const uint64_t ng = cr.n_groups;
    slot->n_groups = ng;
    slot->n_positions = mp;
    slot->cell_group_off.assign((size_t)n_cells + 1, 0);
    slot->group_off.assign(ng + 1, 0);
    slot->kept.assign(ng, 0);
    slot->order.assign(mp, 0);
    OEM_HIP(hipMemcpy(slot->cell_group_off.data(), cr.cell_group_off.p, sizeof(uint64_t) * ((size_t)n_cells + 1), hipMemcpyDeviceToHost));
    OEM_HIP(hipMemcpy(slot->group_off.data(), cr.group_off.p, sizeof(uint64_t) * (ng + 1), hipMemcpyDeviceToHost));
    {
        DevBuf<uint64_t> d_order64;
        OEM_TRY(dev_alloc(&d_order64.p, mp, nullptr));
        hipLaunchKernelGGL(k_order_compose64, grid_of(mp), dim3(kBT), 0, nullptr, mp, (const uint32_t *)cr.order.p,
                           (const uint64_t *)(a->gidx.p + r0), d_order64.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpy(slot->order.data(), d_order64.p, sizeof(uint64_t) * mp, hipMemcpyDeviceToHost));
    }
    RecordsGroup rg;
    rg.n_groups = ng;
    rg.cell_group_off = slot->cell_group_off.data();
    rg.n_cells = n_cells;
    rg.first_cell = cell0;
    rg.out_kept = slot->kept.data();
    rg.out_tables = out->tables.data();
    rg.blk = &out->blk;
    rg.infos = out->infos.data();

    FilterResult r;
    FilterCells fc;
    bool host = rf.host_only;
    if (!host) {
        DevBuf<oem_aln_record> d_sorted;
        const oem_aln_record *d_recs = a->rec.p + r0;
        if (env.mode == kCollateSort || mp != m) { // (the adjacent cut's order is the identity until positions are dropped)
            OEM_TRY(dev_alloc(&d_sorted.p, mp, nullptr));
            OEM_TRY(records_gather(mp, cr.order.p, a->rec.p + r0, d_sorted.p));
            d_recs = d_sorted.p;
        }
        fc.n_cells = n_cells;
        fc.first_cell = cell0;
        OEM_TRY(filter_device_resident(who, rf.f, rf.txp_len.data(), env.n_txps, rf.tab, d_recs, (const unsigned long long *)cr.group_off.p, ng,
                                       (const unsigned long long *)cr.cell_group_off.p, run.cov != nullptr || keep, &r, &fc));
        if (r.bad_ref_record != kNoRecord) { // a collated position of the group: the caller knows its records by their session index
            oem_aln_record rec;
            OEM_HIP(hipMemcpy(&rec, d_recs + r.bad_ref_record, sizeof rec, hipMemcpyDeviceToHost));
            return bad_ref(slot->order[r.bad_ref_record], rec.ref_id);
        }
        host = r.host_rerun;
    }
    if (host) { // the host loop: the group's records come down and are gathered here
        std::vector<uint32_t> order(mp); // (a UMI session: the deduplicated order)
        std::vector<oem_aln_record> recs(m), sorted(mp);
        OEM_HIP(hipMemcpy(order.data(), cr.order.p, sizeof(uint32_t) * mp, hipMemcpyDeviceToHost));
        OEM_HIP(hipMemcpy(recs.data(), a->rec.p + r0, sizeof(oem_aln_record) * m, hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < mp; ++k) {
            sorted[k] = recs[order[k]];
            if (sorted[k].ref_id >= env.n_txps) return bad_ref(slot->order[k], sorted[k].ref_id);
        }
        recs = std::vector<oem_aln_record>();
        rg.records = sorted.data();
        rg.group_off = slot->group_off.data();
        OEM_TRY(records_group_host(who, run, rf, rg, batched));
        slot->done = true;
        return OEM_OK;
    }
    tm.lap("barcodes: gather + filter");
    cr.order.reset();
    cr.group_off.reset();
    cr.cell_group_off.reset();
    OEM_TRY(records_group_filtered(run, rg, r, fc, batched));
    tm.lap("barcodes: group run");
    slot->done = true;
    return OEM_OK;
}

// One batch on the queue's worker (oem_stage_queue.h), in ticket order.  skip: this part is cancelled or the batch was
// never staged; a stuck session skips too.  The queue takes the staging back and the records out of the budget behind this.
void BarcodesStream::process(Batch &b, bool skip)
{
    if (hipSetDevice(env.device) != hipSuccess) set_stuck(OEM_ERR_HIP, "oem_cells_stream: the parse worker could not select its device");
    std::string msg;
    {
        std::lock_guard<std::mutex> lk(mu);
        skip = skip || cancel; // (set before the queue's own flag: cut_groups may have dropped the arena on it already)
    }
    if (skip || env.sticky(&msg) != OEM_OK) return;
    int rc = OEM_OK;
    try {
        rc = run_batch(b);
    } catch (const std::bad_alloc &) {
        rc = fail(OEM_ERR_OOM, "oem_cells_stream: host allocation failed in the parse worker");
    } catch (const std::exception &e) {
        rc = fail(OEM_ERR_STATE, "oem_cells_stream: %s", e.what());
    }
    if (rc != OEM_OK) { // sticky, with everything released
        msg = last_error_text();
        arena.reset();
        carry.reset();
        intern.release();
        release_whitelist();
        set_stuck(rc, msg.c_str());
    }
}

void barcodes_stream_table_info(BarcodesStream *b, uint64_t *arena_peak, uint64_t *misses, uint64_t *slots)
{
    std::lock_guard<std::mutex> lk(b->mu);
    *arena_peak = b->any_order ? b->arena_peak : 0; // (a UMI session: with the arena's UMIs and their offsets)
    *misses = b->any_order ? b->info_misses : 0;
    *slots = b->any_order ? b->info_slots : 0;
}

int barcodes_stream_create(const BarcodesEnv &env, bool any_order, BarcodesStream **out)
{
    std::unique_ptr<BarcodesStream> b(new BarcodesStream(env));
    b->any_order = any_order;
    if (any_order) {
        OEM_HIP(hipSetDevice(env.device));
        OEM_TRY(b->intern.init());
        b->info_slots = b->intern.capacity;
    }
    BarcodesStream *raw = b.get();
    raw->q.start([raw](Batch &bt, bool skip) { raw->process(bt, skip); });
    *out = b.release();
    return OEM_OK;
}

int barcodes_stream_push(BarcodesStream *s, const char *who, const oem_aln_record *records, uint64_t n_records, const uint8_t *barcodes,
                         const uint64_t *barcode_off, const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary,
                         bool with_umis, const uint8_t *umis, const uint64_t *umi_off, uint64_t *out_ticket)
{
    // (set once, before the first push: no lock is needed to read it)
    if (with_umis != s->with_umis)
        return fail(OEM_ERR_STATE, with_umis ? "%s: not a UMI session (oem_cells_stream_set_umis)"
                                             : "%s: a UMI session takes batches through oem_cells_stream_push_barcodes_umis", who);
    // the batch's own checks, on the calling thread, before the session is touched
    const uint64_t n = n_records;
    if (!barcode_off || !name_off) return fail(OEM_ERR_ARG, "%s: barcode_off or name_off is NULL", who);
    if (with_umis && !umi_off) return fail(OEM_ERR_ARG, "%s: umi_off is NULL", who);
    if (n > kCollateMaxBatch) return fail(OEM_ERR_ARG, "%s: %llu records: at most 2^31 - 2 per batch", who, (unsigned long long)n);
    OEM_TRY(check_offsets(who, "barcode_off", barcode_off, n, "record"));
    OEM_TRY(check_offsets(who, "name_off", name_off, n, "record"));
    // (a batch of unmapped records only may come without bytes: a blob is needed where its offsets say it has some)
    if (barcode_off[n] && !barcodes) return fail(OEM_ERR_ARG, "%s: barcodes is NULL and barcode_off[n_records] is not 0", who);
    if (name_off[n] && !names) return fail(OEM_ERR_ARG, "%s: names is NULL and name_off[n_records] is not 0", who);
    if (with_umis) {
        OEM_TRY(check_offsets(who, "umi_off", umi_off, n, "record"));
        if (umi_off[n] && !umis) return fail(OEM_ERR_ARG, "%s: umis is NULL and the UMIs are not all empty", who);
    }
    if (n && !records) return fail(OEM_ERR_ARG, "%s: records is NULL", who);

    Batch lay; // the batch's layout: what the initialiser gives the queue's batch and where the copy puts the arrays
    lay.n_records = n;
    lay.bc_bytes = barcode_off[n];
    lay.name_bytes = name_off[n];
    lay.has_sec = secondary != nullptr && n > 0;
    lay.has_umis = with_umis;
    lay.umi_bytes = with_umis ? umi_off[n] : 0;
    const int rc = s->q.push(
        n, n ? lay.bytes() : 0,
        [&](std::unique_lock<std::mutex> &lk) -> int {
            if (s->stuck_rc != OEM_OK) return fail(s->stuck_rc, "%s", s->stuck_msg.c_str()); // (the first error: before all else)
            std::string msg;
            lk.unlock();
            const int sticky = s->env.sticky(&msg); // (a group's error: the session holds it, under its own lock)
            lk.lock();
            if (sticky != OEM_OK) return fail(sticky, "%s", msg.c_str());
            if (s->closed) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
            return OEM_OK;
        },
        [&](Batch &b) {
            s->ticket_base.push_back(b.rec_base); // (whatever throws, throws here)
            b.bc_bytes = lay.bc_bytes;
            b.name_bytes = lay.name_bytes;
            b.has_sec = lay.has_sec;
            b.has_umis = lay.has_umis;
            b.umi_bytes = lay.umi_bytes;
        },
        [&](char *mem) {
            std::memcpy(mem, records, sizeof(oem_aln_record) * n);
            std::memcpy(mem + lay.at_bc_off(), barcode_off, sizeof(uint64_t) * (n + 1));
            std::memcpy(mem + lay.at_name_off(), name_off, sizeof(uint64_t) * (n + 1));
            if (lay.has_sec) std::memcpy(mem + lay.at_sec(), secondary, n);
            if (lay.bc_bytes) std::memcpy(mem + lay.at_bc(), barcodes, lay.bc_bytes);
            if (lay.name_bytes) std::memcpy(mem + lay.at_names(), names, lay.name_bytes);
            if (lay.has_umis) std::memcpy(mem + lay.at_umi_off(), umi_off, sizeof(uint64_t) * (n + 1));
            if (lay.umi_bytes) std::memcpy(mem + lay.at_umis(), umis, lay.umi_bytes);
        },
        out_ticket);
    if (rc == kStageNoMemory) return fail(OEM_ERR_OOM, "%s: host allocation of the staging memory failed", who); // (sticky: the queue's alloc)
    return rc;
}

int barcodes_stream_set_umis(BarcodesStream *b, const char *who)
{
    std::lock_guard<std::mutex> lk(b->mu);
    if (b->closed || b->cancel) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
    if (b->with_umis) return fail(OEM_ERR_STATE, "%s: the session is a UMI session already", who);
    if (b->q.next_ticket || b->q.pushing) return fail(OEM_ERR_STATE, "%s: a batch has been pushed already", who);
    b->with_umis = true;
    return OEM_OK;
}

void barcodes_stream_umi_info(BarcodesStream *b, uint64_t *dup_reads, uint64_t *dup_records, uint64_t *corrected_reads)
{
    std::lock_guard<std::mutex> lk(b->mu);
    *dup_reads = b->dup_reads;
    *dup_records = b->dup_records;
    *corrected_reads = b->corrected_reads;
}

int barcodes_stream_set_umi_rule(BarcodesStream *b, const char *who, const oem_umi_rule *rule)
{
    if (!rule) return fail(OEM_ERR_ARG, "%s: rule is NULL", who);
    if (rule->correct > 1) return fail(OEM_ERR_ARG, "%s: rule->correct = %u is neither 0 nor 1", who, rule->correct);
    if (rule->gene_of && !rule->n_txps) return fail(OEM_ERR_ARG, "%s: rule->gene_of is given and rule->n_txps is 0", who);
    if (rule->gene_of && rule->n_txps != b->env.n_txps)
        return fail(OEM_ERR_ARG, "%s: rule->n_txps = %u is not the session's n_txps = %u", who, rule->n_txps, b->env.n_txps);
    std::lock_guard<std::mutex> lk(b->mu);
    if (b->closed || b->cancel) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
    if (!b->with_umis) return fail(OEM_ERR_STATE, "%s: not a UMI session (oem_cells_stream_set_umis)", who);
    if (b->rule_set) return fail(OEM_ERR_STATE, "%s: the session has a UMI rule already", who);
    if (b->q.next_ticket || b->q.pushing) return fail(OEM_ERR_STATE, "%s: a batch has been pushed already", who);
    if (rule->gene_of) { // the session's copy, and its upload: the group workers only read it
        std::vector<uint32_t> copy(rule->gene_of, rule->gene_of + rule->n_txps);
        OEM_HIP(hipSetDevice(b->env.device));
        OEM_TRY(dev_alloc(&b->d_gene_of.p, copy.size(), nullptr));
        const hipError_t e = hipMemcpy(b->d_gene_of.p, copy.data(), sizeof(uint32_t) * copy.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            b->d_gene_of.reset();
            return fail(OEM_ERR_HIP, "%s: the upload of gene_of failed: %s", who, hipGetErrorString(e));
        }
        b->gene_of = std::move(copy);
    }
    b->rule_correct = rule->correct;
    b->rule_set = true;
    return OEM_OK;
}

int barcodes_stream_umi_rule_copy(const BarcodesStream *b, const char *who, uint64_t *out_cell_corrected)
{
    if (!b->with_umis || !b->rule_correct) return fail(OEM_ERR_STATE, "%s: not a UMI session under a rule with correct (oem_cells_stream_set_umi_rule)", who);
    if (!b->assembled) return fail(OEM_ERR_STATE, "%s: after a successful oem_cells_stream_finish", who);
    if (!out_cell_corrected) return fail(OEM_ERR_ARG, "%s: out_cell_corrected is NULL", who);
    if (!b->out_cell_corrected.empty())
        std::memcpy(out_cell_corrected, b->out_cell_corrected.data(), sizeof(uint64_t) * b->out_cell_corrected.size());
    return OEM_OK;
}

int barcodes_stream_set_whitelist(BarcodesStream *b, const char *who, const oem_barcode_rule *rule)
{
    OEM_TRY(check_barcode_rule(who, rule));
    if (rule->n_labels >= kBarcodeCorrectedBit)
        return fail(OEM_ERR_ARG, "%s: rule->n_labels = %u: a session's whitelist holds at most 2^31 - 1 labels", who, rule->n_labels);
    std::lock_guard<std::mutex> lk(b->mu);
    if (b->closed || b->cancel) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
    if (!b->any_order)
        return fail(OEM_ERR_STATE,
                    "%s: a collated barcoded session takes no whitelist: its cells are runs of equal barcodes, and corrected barcodes "
                    "would scatter one label over many cells; use the any-order form (oem_cells_stream_set_barcodes_any_order)", who);
    if (b->wl_was_set) return fail(OEM_ERR_STATE, "%s: the session has a whitelist already", who);
    if (b->q.next_ticket || b->q.pushing) return fail(OEM_ERR_STATE, "%s: a batch has been pushed already", who);
    OEM_HIP(hipSetDevice(b->env.device));
    std::unique_ptr<BarcodeWhitelist> wl(new BarcodeWhitelist());
    OEM_TRY(whitelist_build(who, rule, wl.get())); // (a label with a 0 byte, two equal labels: found on the device)
    b->wl_labels.assign(rule->labels, rule->labels + rule->label_off[rule->n_labels]); // the rule's arrays are copied
    b->wl_label_off.assign(rule->label_off, rule->label_off + rule->n_labels + 1);
    b->wl = std::move(wl);
    b->wl_was_set = true;
    return OEM_OK;
}

int barcodes_stream_whitelist_copy(const BarcodesStream *b, const char *who, uint32_t *out_cell_wl_id, uint64_t *out_cell_bc_corrected,
                                   uint64_t *out_counts)
{
    if (!b->wl_was_set) return fail(OEM_ERR_STATE, "%s: not a whitelist session (oem_cells_stream_set_whitelist)", who);
    if (!b->assembled) return fail(OEM_ERR_STATE, "%s: after a successful oem_cells_stream_finish", who);
    if (out_cell_wl_id && !b->out_cell_wl_id.empty())
        std::memcpy(out_cell_wl_id, b->out_cell_wl_id.data(), sizeof(uint32_t) * b->out_cell_wl_id.size());
    if (out_cell_bc_corrected && !b->out_cell_bc_corrected.empty())
        std::memcpy(out_cell_bc_corrected, b->out_cell_bc_corrected.data(), sizeof(uint64_t) * b->out_cell_bc_corrected.size());
    if (out_counts) std::copy(b->wl_counts, b->wl_counts + kBarcodeStatuses, out_counts);
    return OEM_OK;
}

void barcodes_stream_whitelist_info(BarcodesStream *b, uint64_t *rejected, uint64_t *deferred)
{
    std::lock_guard<std::mutex> lk(b->mu);
    *rejected = b->wl_rejected;
    *deferred = b->wl_deferred;
}

int barcodes_stream_umis_copy(const BarcodesStream *b, const char *who, uint64_t *out_cell_dups)
{
    if (!b->with_umis) return fail(OEM_ERR_STATE, "%s: not a UMI session (oem_cells_stream_set_umis)", who);
    if (!b->assembled) return fail(OEM_ERR_STATE, "%s: after a successful oem_cells_stream_finish", who);
    if (!out_cell_dups) return fail(OEM_ERR_ARG, "%s: out_cell_dups is NULL", who);
    if (!b->out_cell_dups.empty()) std::memcpy(out_cell_dups, b->out_cell_dups.data(), sizeof(uint64_t) * b->out_cell_dups.size());
    return OEM_OK;
}

bool barcodes_stream_push_in_flight(BarcodesStream *b) { return b->q.pushes_in_flight() != 0; }

int barcodes_stream_close(BarcodesStream *b, const char *who)
{
    {
        std::lock_guard<std::mutex> lk(b->mu);
        b->closed = true;
    }
    b->q.close(); // (the parse worker runs what is staged)
    std::string msg;
    const int rc = b->env.sticky(&msg);
    if (rc != OEM_OK) return fail(rc, "%s", msg.c_str());
    int rc2 = OEM_OK;
    try {
        OEM_HIP(hipSetDevice(b->env.device));
        if (b->any_order) rc2 = b->finish_any_order(who); // the cells, at last: the arena becomes a collated one
        if (rc2 == OEM_OK) rc2 = b->cut_groups(true);     // the open cell closes with the session
    } catch (const std::bad_alloc &) {
        rc2 = fail(OEM_ERR_OOM, "%s: host allocation failed", who);
    }
    b->arena.reset(); // (the groups hold it)
    b->carry.reset();
    b->intern.release();
    b->release_whitelist();
    if (rc2 != OEM_OK) {
        const std::string m2 = last_error_text();
        b->set_stuck(rc2, m2.c_str());
        return fail(rc2, "%s", m2.c_str());
    }
    return OEM_OK;
}

int barcodes_stream_assemble(BarcodesStream *b, const char *who)
{
    const uint64_t nc = b->n_cells_opened();
    uint64_t n_groups = 0, n_rec = 0, cells = 0;
    for (const auto &sl : b->slots) {
        if (!sl->done) return fail(OEM_ERR_STATE, "%s: a group of cells did not run", who);
        n_groups += sl->n_groups;
        n_rec += sl->n_records;
        cells += sl->n_cells;
    }
    if (cells != nc || n_rec != b->n_survivors)
        return fail(OEM_ERR_STATE, "%s: the groups cover %llu of %llu cells", who, (unsigned long long)cells, (unsigned long long)nc);
    b->out_cell_rec_off.assign(1, 0);
    b->out_cell_rec_off.reserve(nc + 1);
    b->out_cell_group_off.assign(1, 0);
    b->out_cell_group_off.reserve(nc + 1);
    b->out_group_off.reserve(n_groups + 1);
    b->out_order.reserve(n_rec);
    b->out_kept.reserve(n_groups);
    uint64_t rec_base = 0, group_base = 0;
    for (auto &sl : b->slots) {
        // a cell's records from its groups: the cells' first groups, sampled in the group's own group_off
        for (uint32_t c = 1; c <= sl->n_cells; ++c) {
            b->out_cell_rec_off.push_back(rec_base + (sl->cell_pos_off.empty() ? sl->group_off[sl->cell_group_off[c]] : sl->cell_pos_off[c]));
            b->out_cell_group_off.push_back(group_base + sl->cell_group_off[c]);
        }
        for (uint64_t g = 0; g < sl->n_groups; ++g) b->out_group_off.push_back(rec_base + sl->group_off[g]);
        b->out_order.insert(b->out_order.end(), sl->order.begin(), sl->order.end());
        b->out_kept.insert(b->out_kept.end(), sl->kept.begin(), sl->kept.end());
        b->out_cell_dups.insert(b->out_cell_dups.end(), sl->cell_dups.begin(), sl->cell_dups.end());
        b->out_cell_corrected.insert(b->out_cell_corrected.end(), sl->cell_corrected.begin(), sl->cell_corrected.end());
        rec_base += sl->n_positions; // (a UMI session: every later group's place depends on what the earlier ones lost)
        group_base += sl->n_groups;
        sl.reset();
    }
    b->out_group_off.push_back(rec_base);
    b->slots.clear();
    b->assembled = true;
    return OEM_OK;
}

void barcodes_stream_counts(BarcodesStream *b, uint64_t *n_batches, uint64_t *n_records, uint64_t *blocked_us)
{
    std::lock_guard<std::mutex> lk(b->mu);
    *n_batches = b->q.next_ticket;
    *n_records = b->q.total_records;
    *blocked_us = b->q.blocked_us;
}

int barcodes_stream_dims(const BarcodesStream *b, const char *who, uint64_t *n_cells, uint64_t *n_survivors, uint64_t *n_groups,
                         uint64_t *barcode_bytes, uint64_t *n_unmapped)
{
    if (!b->assembled) return fail(OEM_ERR_STATE, "%s: after a successful oem_cells_stream_finish", who);
    if (n_cells) *n_cells = b->n_cells_opened();
    if (n_survivors) *n_survivors = b->out_order.size(); // (a UMI session: the positions that remain)
    if (n_groups) *n_groups = b->out_kept.size();
    if (barcode_bytes) *barcode_bytes = b->labels.size();
    if (n_unmapped) *n_unmapped = b->n_unmapped;
    return OEM_OK;
}

int barcodes_stream_copy(const BarcodesStream *b, const char *who, uint8_t *out_barcodes, uint64_t *out_barcode_off,
                         uint64_t *out_cell_rec_off, uint64_t *out_order, uint64_t *out_group_off, uint64_t *out_cell_group_off,
                         uint32_t *out_kept)
{
    if (!b->assembled) return fail(OEM_ERR_STATE, "%s: after a successful oem_cells_stream_finish", who);
    if ((out_barcodes == nullptr) != (out_barcode_off == nullptr))
        return fail(OEM_ERR_ARG, "%s: out_barcodes and out_barcode_off go together", who);
    auto put = [](auto *dst, const auto &v) {
        if (dst && !v.empty()) std::memcpy(dst, v.data(), sizeof(v[0]) * v.size());
    };
    put(out_barcodes, b->labels);
    put(out_barcode_off, b->label_off);
    put(out_cell_rec_off, b->out_cell_rec_off);
    put(out_order, b->out_order);
    put(out_group_off, b->out_group_off);
    put(out_cell_group_off, b->out_cell_group_off);
    put(out_kept, b->out_kept);
    return OEM_OK;
}

void barcodes_stream_cancel(BarcodesStream *b)
{
    {
        std::lock_guard<std::mutex> lk(b->mu);
        b->cancel = true;
        b->closed = true;
    }
    b->cv_groups.notify_all(); // (the parse worker may be waiting to hand a group over)
    b->q.cancel();
}

void barcodes_stream_destroy(BarcodesStream *b)
{
    if (!b) return;
    barcodes_stream_cancel(b);
    (void)hipSetDevice(b->env.device);
    delete b;
}

} // namespace oem
