// oem_cells_records.hip -- single_cell.rs:104-188 from the alignment records on: oem_em_run_cells_records_sparse, and
// the records-to-group step it shares with the records session (oem_cells_stream.hip).
//
// The reference's worker builds a private InMemoryAlignmentStore per cell with AlignmentFilters::filter, runs the cell's
// coverage model if asked, runs em::em and keeps the entries > 0.  Here a GROUP of consecutive cells goes through those
// stages together, and nothing between its records and its entries exists on the host:
//
//   the cut     the cells are cut into groups BEFORE filtering (cut_cells_groups over the record offsets: a group's
//               records bound the alignments it keeps), so that one or two groups' records are resident at a time and
//               group k + 1's upload and filter run under group k's EM loop, on the workers of run_cells_workers
//   filter      filter_device (oem_filter_device.hip) in its per-cell form: the upload lanes, k_filter_measure with the
//               discard counters summed per cell, the two scans, k_filter_emit, and k_filter_cell_offsets, which samples
//               the scans at the cells' first groups -- the group's cell_row_off and cell_aln_off, on the device
//   the group   the filtered CSR becomes the ResidentCsr of a CellsGroup: u32 row pointers and ids as emitted, as_prob as
//               the f32 weights or, with a coverage model, cells_coverage_group over the filter's coordinates
//   the run     run_cells_group, as for every other group of the per-cell driver, fallbacks included: a batch the tiler
//               declines gets its ids back from their device copy, and only the host layout builder reads arrays back
//
// A group takes the host loop instead (one host builder, cell after cell; the same result) when the filter does: no gap
// table for score_prob_denom, or a mapped score beyond +-2^24 found by the measure pass.
//
// oem_em_run_cells_records_names_sparse takes the worker from its first step, sort_and_parse_barcode_records
// (alignment_parser.rs:170-241): names and records in input order in.  Per group of cells, on the group's worker:
//   collate     collate_resident (oem_collate_device.hip): the group's names go up through the upload lanes, the rounds
//               run, and `order`, the group's group_off and cell_group_off stay on the device; the sort's buffers and the
//               names are released before the records arrive
//   upload      the group's records, in input order, through the same lanes (no kernel behind the chunks)
//   gather      k_records_gather: dst[k] = src[order[k]] over 40-byte records, then the buffer in input order is freed
//   filter      filter_device_resident: one k_filter_measure launch, the scans, k_filter_emit, k_filter_cell_offsets;
//               one scalar (n_groups) and the n_cells + 1 cell offsets are what the host sees
// and the group goes on as above.  The host loop, when the group takes it, gets order and group_off down and gathers
// the group's records on the host.
//
// oem_em_run_cells_records_barcodes_sparse takes records that are not collated at all (oem_collate.h's barcode rule; the
// reference requires a barcode's records to be adjacent, single_cell.rs:196-213).  Once per call: collate_barcodes_resident
// leaves order_bc and cell_rec_off on the device; names (validated behind their upload chunks, so a bad name is named
// by its input index), flags and records go up once, in input order, and stay; one scan of the name lengths in order_bc
// order gives every record's place in its group's gathered blob.  Then the groups of cells, as above, except that
//   collate     k_names_gather / k_flags_gather put the group's names and flags into a dense blob in order_bc order, and
//               collate_resident runs in its device form (no lanes, no validate pass) with positions for record indices
//   compose     k_order_compose: order[k] = order_bc[r0 + order[k]], the record's index in the caller's input
//   gather      k_records_gather straight from the whole-input buffer, under either mode (order_bc is no identity)
//
// oem_em_run_cells_records_umis_sparse is that call with the UMIs resident too (umis_upload, oem_dedup_umis.hip).  Between a
// group's collate and its compose run dedup_mark and, where it found duplicates, dedup_compact (oem_collate.h's UMI rule):
// order, group_off and cell_group_off are replaced by the deduplicated ones, so the duplicates' records are never
// gathered and the filter sees the survivors only.  A group's place in the call's order is then known only when every
// group before it is done: its order waits in its slot like kept and group_off.
//
// oem_em_run_cells_records_whitelist_sparse is that call on RAW barcodes: order_bc and cell_rec_off come from
// correct_barcodes_resident (oem_barcode_correct.hip) and describe the ACCEPTED records only.  The whole input still goes
// up once and in input order, but from there on the positions (cro[n_cells], accepted records) and the records (n,
// resident, indexed by order_bc's entries) are two numbers; a rejected record is never gathered, and because nothing of
// it may be looked at, names and UMIs are validated over order_bc instead of behind their upload chunks.
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "oem_barcode_correct.h"
#include "oem_cells.h"
#include "oem_cells_barcodes_stream.h"
#include "oem_collate_device.h"
#include "oem_filter_device.h"

namespace oem {
namespace {

// The filtered CSR of the last group that went through the device pass, kept by the test-only library when asked to
// (OEM_TEST_KEEP_RECORDS_CSR=1) for oem_debug_cells_records_last_csr.
struct KeptCsr {
    std::mutex mu;
    std::vector<uint32_t> row_ptr, tid, start, end;
    std::vector<float> as_prob;
    std::vector<uint64_t> cell_row_off;
} g_kept;

int keep_csr(const FilterResult &r, const FilterCells &fc)
{
    std::lock_guard<std::mutex> lk(g_kept.mu);
    g_kept.row_ptr.resize(r.n_rows + 1);
    g_kept.tid.resize(r.nnz);
    g_kept.start.resize(r.nnz);
    g_kept.end.resize(r.nnz);
    g_kept.as_prob.resize(r.nnz);
    g_kept.cell_row_off = fc.cell_row_off;
    OEM_HIP(hipMemcpy(g_kept.row_ptr.data(), r.row_ptr32.p, sizeof(uint32_t) * (r.n_rows + 1), hipMemcpyDeviceToHost));
    if (r.nnz) {
        OEM_HIP(hipMemcpy(g_kept.tid.data(), r.tid.p, sizeof(uint32_t) * r.nnz, hipMemcpyDeviceToHost));
        OEM_HIP(hipMemcpy(g_kept.start.data(), r.start.p, sizeof(uint32_t) * r.nnz, hipMemcpyDeviceToHost));
        OEM_HIP(hipMemcpy(g_kept.end.data(), r.end.p, sizeof(uint32_t) * r.nnz, hipMemcpyDeviceToHost));
        OEM_HIP(hipMemcpy(g_kept.as_prob.data(), r.as_prob.p, sizeof(float) * r.nnz, hipMemcpyDeviceToHost));
    }
    return OEM_OK;
}

// Host arrays for the host layout builder, fetched only when it asks (ResidentCsr::host_row_ptr / host_tid).  The
// pointers are the group's device buffers: the row pointers belong to the store by then and are never rewritten, the
// ids are the copy the filter's were saved to before the batch relabelled them.
struct HostArrays {
    const uint32_t *d_row_ptr = nullptr, *d_tid = nullptr;
    uint64_t n_reads = 0, nnz = 0;
    std::vector<uint64_t> rp;
    std::vector<uint32_t> tid;
    static const uint64_t *get_row_ptr(void *ctx)
    {
        HostArrays *h = (HostArrays *)ctx;
        try {
            std::vector<uint32_t> rp32(h->n_reads + 1);
            if (hipMemcpy(rp32.data(), h->d_row_ptr, sizeof(uint32_t) * rp32.size(), hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
            h->rp.assign(rp32.begin(), rp32.end());
        } catch (...) {
            return nullptr;
        }
        return h->rp.data();
    }
    static const uint32_t *get_tid(void *ctx)
    {
        HostArrays *h = (HostArrays *)ctx;
        try {
            h->tid.resize(h->nnz ? h->nnz : 1);
            if (h->nnz && hipMemcpy(h->tid.data(), h->d_tid, sizeof(uint32_t) * h->nnz, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
        } catch (...) {
            return nullptr;
        }
        return h->tid.data();
    }
};

// The host loop of a group: one host builder takes the cells one after the other (a cell's table is what its groups
// added), and the group runs from the builder's arrays like a slice of a one-call run.
int run_records_group_host(const char *who, const CellsRun &run, const RecordsFilter &rf, const RecordsGroup &rg, bool *batched)
{
    const uint32_t nc = rg.n_cells;
    oem_builder hb;
    hb.f = rf.f;
    hb.txp_len = rf.txp_len;
    std::vector<uint64_t> cro((size_t)nc + 1, 0), cao((size_t)nc + 1, 0);
    for (uint32_t c = 0; c < nc; ++c) {
        const uint64_t g0 = rg.cell_group_off[c], g1 = rg.cell_group_off[c + 1];
        for (uint64_t i = rg.group_off[g0]; i < rg.group_off[g1]; ++i) // (the device pass's message: the cell, the record)
            if (!(rg.records[i].flags & OEM_REC_UNMAPPED) && rg.records[i].ref_id >= run.n_txps)
                return fail(OEM_ERR_ARG, "%s: cell %llu: record %llu: ref_id %u is not below n_txps", who,
                            (unsigned long long)(rg.first_cell + c), (unsigned long long)(rg.first_record + i), rg.records[i].ref_id);
        const oem_discard_table before = hb.dt;
        OEM_TRY(add_groups_host(&hb, rg.records, rg.group_off + g0, g1 - g0, rg.out_kept ? rg.out_kept + g0 : nullptr, who));
        for (int k = 0; k < kFilterCounters; ++k) (&rg.out_tables[c].discard_5p)[k] = (&hb.dt.discard_5p)[k] - (&before.discard_5p)[k];
        cro[c + 1] = hb.row_ptr.size() - 1;
        cao[c + 1] = hb.tid.size();
    }
    if (hb.tid.size() >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: a group of cells needs fewer than 2^32 alignments", who);
    ResidentCsr res;
    CellsGroup cg;
    cg.n_cells = nc;
    cg.n_reads = hb.row_ptr.size() - 1;
    cg.nnz = hb.tid.size();
    cg.first_cell = rg.first_cell;
    cg.cell_row_off = cro.data();
    cg.cell_aln_off = cao.data();
    cg.row_ptr = hb.row_ptr.data();
    cg.tid = hb.tid.data();
    cg.as_prob = hb.as_prob.data();
    if (run.cov) {
        cg.aln_start = hb.start.data();
        cg.aln_end = hb.end.data();
        cg.resident = &res;
    }
    cg.blk = rg.blk;
    cg.infos = rg.infos;
    cg.launch = rg.launch;
    return run_cells_group(run, cg, batched);
}

// The group behind its device filter pass (r, fc): kept and the tables go to the caller, the filtered CSR becomes the
// group's resident one, and the group runs.  Consumes r.
int run_filtered_group(const CellsRun &run, const RecordsGroup &rg, FilterResult &r, FilterCells &fc, bool keep, bool *batched)
{
    const uint32_t nc = rg.n_cells;
    if (rg.out_kept && rg.n_groups)
        OEM_HIP(hipMemcpy(rg.out_kept, r.n_kept.p, sizeof(uint32_t) * rg.n_groups, hipMemcpyDeviceToHost));
    std::copy(fc.tables.begin(), fc.tables.end(), rg.out_tables);
    r.n_kept.reset();
    r.txp_len.reset();
    r.strand.reset();
    if (keep) OEM_TRY(keep_csr(r, fc));

    // the filtered CSR as the group's resident one; the ids once more, as the filter wrote them
    ResidentCsr res;
    res.row_ptr = r.row_ptr32.p;
    r.row_ptr32.p = nullptr;
    res.tid = r.tid.p;
    r.tid.p = nullptr;
    DevBuf<uint32_t> d_tid_orig;
    OEM_TRY(dev_alloc(&d_tid_orig.p, r.nnz, nullptr));
    if (r.nnz) OEM_HIP(hipMemcpy(d_tid_orig.p, res.tid, sizeof(uint32_t) * r.nnz, hipMemcpyDeviceToDevice));
    if (!run.cov) {
        res.w32 = r.as_prob.p;
        r.as_prob.p = nullptr;
        r.start.reset();
        r.end.reset();
    }
    HostArrays ha;
    ha.d_row_ptr = res.row_ptr;
    ha.d_tid = d_tid_orig.p;
    ha.n_reads = r.n_rows;
    ha.nnz = r.nnz;
    res.host_row_ptr = &HostArrays::get_row_ptr;
    res.host_tid = &HostArrays::get_tid;
    res.host_row_ptr_ctx = &ha;

    CellsGroup cg; // no host arrays at all: the offsets of the cells are the only thing that came back
    cg.n_cells = nc;
    cg.n_reads = r.n_rows;
    cg.nnz = r.nnz;
    cg.first_cell = rg.first_cell;
    cg.cell_row_off = fc.cell_row_off.data();
    cg.cell_aln_off = fc.cell_aln_off.data();
    cg.resident = &res;
    cg.d_cell_row_off = fc.d_cell_row_off.p;
    cg.d_tid_orig = d_tid_orig.p;
    if (run.cov) {
        cg.d_aln_start = r.start.p;
        cg.d_aln_end = r.end.p;
        cg.d_as_prob = r.as_prob.p;
    }
    cg.blk = rg.blk;
    cg.infos = rg.infos;
    cg.launch = rg.launch;
    return run_cells_group(run, cg, batched);
}


// ---- names and records in input order (oem_em_run_cells_records_names_sparse)
constexpr int kGT = 256;                           // k_records_gather's workgroup
constexpr uint64_t kRecordWords = 5;               // a record as aligned 8-byte words
constexpr uint64_t kUploadChunkRecords = 1ull << 20; // records per upload chunk of the lanes (40 MiB)
constexpr uint64_t kGroupNameBytes = 16ull << 30;  // name bytes a group of cells may hold (testing build: OEM_CELLS_GROUP_NAME_BYTES)
static_assert(sizeof(oem_aln_record) == 8 * kRecordWords && alignof(oem_aln_record) == 8, "a record is five aligned words");

// dst[k] = src[order[k] - order_base] over the m records of a group, one lane per 8-byte word: word j of the
// destination is word j % 5 of record j / 5.  The stores are lane i at base + 8 i, fully coalesced; the loads are runs of
// five lanes on 40 contiguous bytes, scattered at that granularity, which is all the source allows.  (One lane per
// record would make both sides 8 bytes at a stride of 40.)
// order[k] = order_bc[order[k]]: a group's collated positions become the records' indices in the caller's input
__global__ __launch_bounds__(kGT) void k_order_compose(uint64_t m, const uint32_t *__restrict__ order_bc, uint32_t *__restrict__ order)
{
    const uint64_t k = (uint64_t)blockIdx.x * kGT + threadIdx.x;
    if (k < m) order[k] = order_bc[order[k]];
}

// dst[c] = src[at[c]]: the gathered name offsets at the cells' first records
__global__ __launch_bounds__(kGT) void k_sample_offsets(uint64_t n, const uint64_t *__restrict__ at, const uint64_t *__restrict__ src,
                                                         uint64_t *__restrict__ dst)
{
    const uint64_t c = (uint64_t)blockIdx.x * kGT + threadIdx.x;
    if (c < n) dst[c] = src[at[c]];
}

__global__ __launch_bounds__(kGT) void k_records_gather(uint64_t n_words, const uint32_t *__restrict__ order, uint32_t order_base,
                                                         const uint64_t *__restrict__ src, uint64_t *__restrict__ dst)
{
    const uint64_t j = (uint64_t)blockIdx.x * kGT + threadIdx.x;
    if (j >= n_words) return;
    const uint64_t k = j / kRecordWords, w = j - k * kRecordWords;
    dst[j] = src[(uint64_t)(order[k] - order_base) * kRecordWords + w];
}

// What a call of the names form shares between its groups, and where a group leaves what the caller asked for: the
// groups' numbers in the call are known only when every group before has been collated, so kept and group_off wait in
// the group's slot until the workers have joined.
// The whole input of the barcodes form on the device, in the caller's order, and the barcode collation's result.
struct ResidentInput {
    const oem_aln_record *records = nullptr;
    const uint8_t *names = nullptr, *sec = nullptr; // sec: NULL without flags
    const uint64_t *name_off = nullptr;             // n_records + 1
    const uint32_t *order_bc = nullptr;             // n_records
    const uint64_t *gathered_off = nullptr;         // n_records + 1: the names' offsets in order_bc order
    const uint64_t *cell_name_off = nullptr;        // HOST, n_cells + 1: gathered_off at the cells' first records
    const UmiInput *umi = nullptr;                  // the UMIs form: the groups are deduplicated behind their name collation
};
struct NamesCall {
    CollateInput in;
    const ResidentInput *dev = nullptr;             // the barcodes form; in.cell_rec_off is then the barcode collation's
    const oem_aln_record *records = nullptr;
    uint32_t *out_order = nullptr;
    bool want_group_off = false, want_kept = false;
};
struct NamesSlot {
    uint64_t n_groups = 0;
    std::vector<uint64_t> group_off, cell_group_off; // from 0: n_groups + 1 (if asked for), n_cells + 1
    std::vector<uint32_t> kept;                      // n_groups (if asked for)
    // the UMIs form, whose groups' places in the call's order are known only when the workers have joined
    uint64_t n_positions = 0;                        // the positions of the group's deduplicated order
    std::vector<uint32_t> order;                     // n_positions (if asked for)
    std::vector<uint64_t> cell_pos_off, cell_dups;   // from 0: n_cells + 1; n_cells
    std::vector<uint64_t> cell_corrected;            // n_cells (under a UMI rule: the cells' corrected groups)
};

// The cells [c0, c1) of the call: collate, gather, filter and run.  rg: the group's place and outputs (records,
// offsets and out_kept are filled in here).
int run_names_group(const char *who, const CellsRun &run, const RecordsFilter &rf, const NamesCall &nc, uint32_t c0, uint32_t c1,
                    RecordsGroup rg, NamesSlot *slot, bool *batched)
{
    *batched = false;
    StageTimer tm;
    const uint32_t n_cells = c1 - c0;
    const uint64_t r0 = nc.in.cell_rec_off[c0], m = nc.in.cell_rec_off[c1] - r0;
    const bool keep = knob("OEM_TEST_KEEP_RECORDS_CSR", 0) != 0;
    OEM_TRY(ensure_device(run.device));
    slot->cell_group_off.assign((size_t)n_cells + 1, 0);
    if (nc.want_group_off) slot->group_off.assign(1, 0);
    rg.first_cell = c0;
    rg.first_record = r0;
    rg.n_cells = n_cells;
    rg.cell_group_off = slot->cell_group_off.data();
    const bool dedup = nc.dev && nc.dev->umi;
    uint64_t mp = m;           // the positions of the group's order: fewer than its records once duplicates are dropped
    std::vector<uint64_t> cpo; // then also the cells' first positions in it, from 0
    if (dedup) {
        slot->cell_pos_off.assign((size_t)n_cells + 1, 0);
        slot->cell_dups.assign(n_cells, 0);
        slot->cell_corrected.assign(n_cells, 0);
    }
    if (m == 0) { // cells without records: no groups, and the run of cells without reads
        const uint64_t zero = 0;
        rg.group_off = &zero;
        rg.n_groups = 0;
        return run_records_group(who, run, rf, rg, batched);
    }

    CollateResident cr;
    double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (nc.dev) { // the group's names and flags out of the resident input, in order_bc order; positions, then input indices
        const ResidentInput &dv = *nc.dev;
        const uint64_t b0 = dv.cell_name_off[c0], nb = dv.cell_name_off[c1] - b0;
        DevBuf<uint8_t> d_gnames, d_gsec;
        OEM_TRY(dev_alloc(&d_gnames.p, nb + 16, nullptr));
        if (dv.sec) OEM_TRY(dev_alloc(&d_gsec.p, ((m + 8) / 8) * 8, nullptr));
        OEM_TRY(gather_names(dv.order_bc + r0, m, dv.names, dv.name_off, dv.gathered_off + r0, b0, nb, d_gnames.p, dv.sec, d_gsec.p));
        tm.lap("barcodes: names gather");
        CollateInput in = nc.in;
        in.d_names = d_gnames.p;
        in.d_name_off = dv.gathered_off + r0;
        in.d_off_base = b0;
        in.d_n_bytes = nb;
        in.d_secondary = d_gsec.p;
        OEM_TRY(collate_resident(in, c0, c1, 0, 0, 0, info, &cr));
        if (dedup) { // the duplicates leave the collation here: their records are never gathered
            d_gnames.reset();
            d_gsec.reset();
            tm.lap("names: collate");
            UmiMarks mk;
            OEM_TRY(dedup_mark(*dv.umi, cr.order.p, dv.order_bc + r0, cr.group_off.p, cr.n_groups, cr.cell_group_off.p, n_cells, 0, &mk,
                               slot->cell_dups.data(), slot->cell_corrected.data()));
            if (mk.n_dups) {
                cpo.resize((size_t)n_cells + 1);
                OEM_TRY(dedup_compact(mk, m, n_cells, &cr, &mp, cpo.data()));
                slot->cell_pos_off = cpo;
            } else {
                for (uint32_t c = 0; c <= n_cells; ++c) slot->cell_pos_off[c] = nc.in.cell_rec_off[c0 + c] - r0;
            }
            tm.lap("umis: dedup");
        }
        hipLaunchKernelGGL(k_order_compose, dim3((uint32_t)((mp + kGT - 1) / kGT)), dim3(kGT), 0, nullptr, mp, dv.order_bc + r0, cr.order.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipStreamSynchronize(nullptr));
    } else {
        OEM_TRY(collate_resident(nc.in, c0, c1, r0, 0, 0, info, &cr));
    }
    tm.lap("names: collate");
    const uint64_t ng = cr.n_groups;
    slot->n_groups = ng;
    OEM_HIP(hipMemcpy(slot->cell_group_off.data(), cr.cell_group_off.p, sizeof(uint64_t) * ((size_t)n_cells + 1), hipMemcpyDeviceToHost));
    slot->n_positions = mp;
    if (nc.out_order && dedup) {
        slot->order.resize(mp);
        OEM_HIP(hipMemcpy(slot->order.data(), cr.order.p, sizeof(uint32_t) * mp, hipMemcpyDeviceToHost));
    } else if (nc.out_order)
        OEM_HIP(hipMemcpy(nc.out_order + r0, cr.order.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    // a record's cell from its position in the group's order: the sort stays inside cells
    auto cell_at = [&](uint64_t k) -> uint64_t {
        if (!cpo.empty()) return c0 + (uint64_t)(std::upper_bound(cpo.begin(), cpo.end(), k) - cpo.begin()) - 1;
        const uint64_t *cro = nc.in.cell_rec_off;
        return (uint64_t)(std::upper_bound(cro + c0, cro + c1 + 1, r0 + k) - cro) - 1;
    };
    if (nc.want_group_off) {
        slot->group_off.resize(ng + 1);
        OEM_HIP(hipMemcpy(slot->group_off.data(), cr.group_off.p, sizeof(uint64_t) * (ng + 1), hipMemcpyDeviceToHost));
    }
    if (nc.want_kept) slot->kept.assign(ng, 0);
    rg.n_groups = ng;
    rg.out_kept = nc.want_kept ? slot->kept.data() : nullptr;
    const bool sorting = nc.in.mode == kCollateSort;

    FilterResult r;
    FilterCells fc;
    bool host = rf.host_only;
    if (!host) {
        DevBuf<oem_aln_record> d_in, d_sorted;
        if (!nc.dev) {
            OEM_TRY(dev_alloc(&d_in.p, m, nullptr));
            OEM_TRY(upload_records(nc.records + r0, m, d_in.p));
        }
        const oem_aln_record *d_recs = d_in.p;
        if (sorting || nc.dev) { // (the adjacent cut's order is the identity; with barcodes it is order_bc's slice)
            OEM_TRY(dev_alloc(&d_sorted.p, mp, nullptr));
            const uint64_t n_words = mp * kRecordWords;
            hipLaunchKernelGGL(k_records_gather, dim3((uint32_t)((n_words + kGT - 1) / kGT)), dim3(kGT), 0, nullptr, n_words,
                               (const uint32_t *)cr.order.p, (uint32_t)(nc.dev ? 0 : r0),
                               (const uint64_t *)(nc.dev ? nc.dev->records : d_in.p), (uint64_t *)d_sorted.p);
            OEM_HIP(hipGetLastError());
            OEM_HIP(hipStreamSynchronize(nullptr));
            d_in.reset(); // the group holds its records twice only for the length of the gather
            d_recs = d_sorted.p;
        }
        fc.n_cells = n_cells;
        fc.first_cell = c0;
        fc.first_record = r0;
        OEM_TRY(filter_device_resident(who, rf.f, rf.txp_len.data(), run.n_txps, rf.tab, d_recs, (const unsigned long long *)cr.group_off.p,
                                       ng, (const unsigned long long *)cr.cell_group_off.p, run.cov != nullptr || keep, &r, &fc));
        if (r.bad_ref_record != kNoRecord) { // a collated index: the caller knows its records by their input index
            uint32_t at = 0;
            OEM_HIP(hipMemcpy(&at, cr.order.p + r.bad_ref_record, sizeof at, hipMemcpyDeviceToHost));
            const uint64_t c = cell_at((uint64_t)r.bad_ref_record);
            return fail(OEM_ERR_ARG, "%s: cell %llu: record %llu: ref_id %u is not below n_txps", who, (unsigned long long)c,
                        (unsigned long long)at, nc.records[at].ref_id);
        }
        host = r.host_rerun;
    }
    if (host) { // the host loop: order and group_off come down, the host gathers the group's records
        std::vector<uint32_t> order(mp);
        std::vector<uint64_t> goff(ng + 1);
        OEM_HIP(hipMemcpy(order.data(), cr.order.p, sizeof(uint32_t) * mp, hipMemcpyDeviceToHost));
        OEM_HIP(hipMemcpy(goff.data(), cr.group_off.p, sizeof(uint64_t) * (ng + 1), hipMemcpyDeviceToHost));
        std::vector<oem_aln_record> sorted(mp);
        for (uint64_t k = 0; k < mp; ++k) {
            sorted[k] = nc.records[order[k]];
            if (!(sorted[k].flags & OEM_REC_UNMAPPED) && sorted[k].ref_id >= run.n_txps) {
                const uint64_t c = cell_at(k);
                return fail(OEM_ERR_ARG, "%s: cell %llu: record %llu: ref_id %u is not below n_txps", who, (unsigned long long)c,
                            (unsigned long long)order[k], sorted[k].ref_id);
            }
        }
        rg.records = sorted.data();
        rg.group_off = goff.data();
        return run_records_group_host(who, run, rf, rg, batched);
    }
    tm.lap("names: upload + gather + filter");
    cr.order.reset();
    cr.group_off.reset();
    cr.cell_group_off.reset();
    const int rc = run_filtered_group(run, rg, r, fc, keep, batched);
    tm.lap("names: group run");
    return rc;
}

// The groups' numbers in the call, once every group's count is known: the slots into the caller's arrays (each or NULL).
void names_call_outputs(const std::vector<std::pair<uint32_t, uint32_t>> &groups, const std::vector<NamesSlot> &slots,
                        const uint64_t *cell_rec_off, uint64_t n_records, uint64_t *out_group_off, uint64_t *out_n_groups,
                        uint64_t *out_cell_group_off, uint32_t *out_kept)
{
    uint64_t group_base = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
        const uint32_t c0 = groups[g].first, c1 = groups[g].second;
        const NamesSlot &sl = slots[g];
        if (out_cell_group_off)
            for (uint32_t c = c0; c <= c1; ++c) out_cell_group_off[c] = group_base + sl.cell_group_off[c - c0];
        if (out_group_off)
            for (uint64_t k = 0; k < sl.n_groups; ++k) out_group_off[group_base + k] = cell_rec_off[c0] + sl.group_off[k];
        if (out_kept && sl.n_groups) std::memcpy(out_kept + group_base, sl.kept.data(), sizeof(uint32_t) * sl.n_groups);
        group_base += sl.n_groups;
    }
    if (out_cell_group_off && groups.empty()) out_cell_group_off[0] = 0;
    if (out_group_off) out_group_off[group_base] = n_records;
    if (out_n_groups) *out_n_groups = group_base;
}

// The same for the UMIs form, whose groups' first positions are known only now too: a group's order, its cells' first
// positions and their duplicate counts wait in its slot.
void umis_call_outputs(const std::vector<std::pair<uint32_t, uint32_t>> &groups, const std::vector<NamesSlot> &slots, uint32_t *out_order,
                       uint64_t *out_n_survivors, uint64_t *out_cell_rec_off, uint64_t *out_group_off, uint64_t *out_n_groups,
                       uint64_t *out_cell_group_off, uint32_t *out_kept, uint64_t *out_cell_dups, uint64_t *out_cell_corrected)
{
    uint64_t group_base = 0, pos_base = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
        const uint32_t c0 = groups[g].first, c1 = groups[g].second;
        const NamesSlot &sl = slots[g];
        for (uint32_t c = c0; c <= c1; ++c) {
            if (out_cell_group_off) out_cell_group_off[c] = group_base + sl.cell_group_off[c - c0];
            if (out_cell_rec_off) out_cell_rec_off[c] = pos_base + sl.cell_pos_off[c - c0];
        }
        if (out_group_off)
            for (uint64_t k = 0; k < sl.n_groups; ++k) out_group_off[group_base + k] = pos_base + sl.group_off[k];
        if (out_kept && sl.n_groups) std::memcpy(out_kept + group_base, sl.kept.data(), sizeof(uint32_t) * sl.n_groups);
        if (out_order && sl.n_positions) std::memcpy(out_order + pos_base, sl.order.data(), sizeof(uint32_t) * sl.n_positions);
        if (out_cell_dups) std::copy(sl.cell_dups.begin(), sl.cell_dups.end(), out_cell_dups + c0);
        if (out_cell_corrected) std::copy(sl.cell_corrected.begin(), sl.cell_corrected.end(), out_cell_corrected + c0);
        group_base += sl.n_groups;
        pos_base += sl.n_positions;
    }
    if (groups.empty()) {
        if (out_cell_group_off) out_cell_group_off[0] = 0;
        if (out_cell_rec_off) out_cell_rec_off[0] = 0;
    }
    if (out_group_off) out_group_off[group_base] = pos_base;
    if (out_n_groups) *out_n_groups = group_base;
    if (out_n_survivors) *out_n_survivors = pos_base;
}

// The cut of the records call (a group's records bound its reads and alignments), and then what the collation adds: a
// group is one collation batch, so it also stays within a batch's records and within the name bytes of a group.
// name_byte_off (n_cells + 1): the cells' first name bytes.
template <typename NameBytes>
std::vector<std::pair<uint32_t, uint32_t>> cut_names_groups(const uint64_t *cell_rec_off, uint32_t n_cells, uint32_t n_txps, NameBytes &&cell_bytes)
{
    std::vector<std::pair<uint32_t, uint32_t>> groups;
    const uint64_t max_records = collate_batch_records(), max_bytes = (uint64_t)knob("OEM_CELLS_GROUP_NAME_BYTES", (long)kGroupNameBytes);
    for (const auto &g : cut_cells_groups(cell_rec_off, n_cells, nullptr, n_txps)) {
        uint32_t c0 = g.first;
        while (c0 < g.second) {
            uint32_t c1 = c0 + 1;
            while (c1 < g.second && cell_rec_off[c1 + 1] - cell_rec_off[c0] <= max_records && cell_bytes(c1 + 1) - cell_bytes(c0) <= max_bytes)
                ++c1;
            groups.emplace_back(c0, c1);
            c0 = c1;
        }
    }
    return groups;
}

thread_local double g_cells_barcodes_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};

} // namespace

void cells_barcodes_last_call(double *out8) { std::memcpy(out8, g_cells_barcodes_last, sizeof g_cells_barcodes_last); }

// the two ends of run_names_group for the barcoded session (oem_cells_barcodes_stream.hip), whose groups are cut from
// its device arena
int records_group_filtered(const CellsRun &run, const RecordsGroup &rg, FilterResult &r, FilterCells &fc, bool *batched)
{
    return run_filtered_group(run, rg, r, fc, knob("OEM_TEST_KEEP_RECORDS_CSR", 0) != 0, batched);
}
int records_group_host(const char *who, const CellsRun &run, const RecordsFilter &rf, const RecordsGroup &rg, bool *batched)
{
    return run_records_group_host(who, run, rf, rg, batched);
}

// The records [r0, r0 + m) of the caller into d (input order) through the upload lanes.
int upload_records(const oem_aln_record *records, uint64_t m, oem_aln_record *d)
{
    std::vector<uint64_t> cut;
    for (uint64_t r = 0; r < m; r += kUploadChunkRecords) cut.push_back(r);
    cut.push_back(m);
    return filter_upload_measure<oem_aln_record>(records, d, cut.data(), cut.size() - 1, 1, nullptr, [](hipStream_t, uint64_t, uint64_t) {});
}

// k_order_compose and k_records_gather for oem_records_names.hip, on the null stream, which is left idle
int order_compose(uint64_t m, const uint32_t *d_outer, uint32_t *d_order)
{
    if (!m) return OEM_OK;
    hipLaunchKernelGGL(k_order_compose, dim3((uint32_t)((m + kGT - 1) / kGT)), dim3(kGT), 0, nullptr, m, d_outer, d_order);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipStreamSynchronize(nullptr));
    return OEM_OK;
}

int records_gather(uint64_t m, const uint32_t *d_order, const oem_aln_record *d_src, oem_aln_record *d_dst)
{
    if (!m) return OEM_OK;
    const uint64_t n_words = m * kRecordWords;
    hipLaunchKernelGGL(k_records_gather, dim3((uint32_t)((n_words + kGT - 1) / kGT)), dim3(kGT), 0, nullptr, n_words, d_order, 0u,
                       (const uint64_t *)d_src, (uint64_t *)d_dst);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipStreamSynchronize(nullptr));
    return OEM_OK;
}

int records_filter_setup(const char *who, const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps, RecordsFilter *rf)
{
    if (!filters || !txp_len || n_txps == 0) return fail(OEM_ERR_ARG, "%s: bad argument", who);
    rf->f = *filters;
    rf->txp_len.assign(txp_len, txp_len + n_txps);
    rf->host_only = !filter_prob_table(filters->score_prob_denom, rf->tab);
    return OEM_OK;
}

int run_records_group(const char *who, const CellsRun &run, const RecordsFilter &rf, const RecordsGroup &rg, bool *batched)
{
    *batched = false;
    StageTimer tm;
    const uint32_t nc = rg.n_cells;
    const bool keep = knob("OEM_TEST_KEEP_RECORDS_CSR", 0) != 0; // testing build: the hook reads the coordinates too
    OEM_TRY(ensure_device(run.device));
    FilterResult r;
    FilterCells fc;
    bool host = rf.host_only;
    if (!host) {
        fc.cell_group_off = rg.cell_group_off;
        fc.n_cells = nc;
        fc.first_cell = rg.first_cell;
        fc.first_record = rg.first_record;
        OEM_TRY(filter_device(who, rf.f, rf.txp_len.data(), run.n_txps, rf.tab, rg.records, rg.group_off, rg.n_groups, 0,
                              run.cov != nullptr || keep, true, &r, &fc, rg.pinned));
        host = r.host_rerun;
    }
    if (host) return run_records_group_host(who, run, rf, rg, batched);
    tm.lap("records: upload + filter");
    const int rc = run_filtered_group(run, rg, r, fc, keep, batched);
    tm.lap("records: group run");
    return rc;
}

int check_cell_group_off(const char *who, const uint64_t *cell_group_off, uint32_t n_cells, uint64_t n_groups)
{
    if (!cell_group_off) return fail(OEM_ERR_ARG, "%s: cell_group_off is NULL", who);
    if (cell_group_off[0] != 0) return fail(OEM_ERR_ARG, "%s: cell_group_off[0] must be 0", who);
    for (uint32_t c = 0; c < n_cells; ++c)
        if (cell_group_off[c + 1] < cell_group_off[c])
            return fail(OEM_ERR_ARG, "%s: cell_group_off decreases at cell %u", who, c);
    if (cell_group_off[n_cells] != n_groups)
        return fail(OEM_ERR_ARG, "%s: cell_group_off must end at n_groups (%llu, not %llu)", who, (unsigned long long)n_groups,
                    (unsigned long long)cell_group_off[n_cells]);
    return OEM_OK;
}

// test hook (oem_testing.hip): the kept CSR's sizes, then its arrays (any of them may be NULL)
int cells_records_last_csr(uint64_t *dims3, uint32_t *row_ptr, uint32_t *tid, uint32_t *as_prob_bits, uint32_t *start,
                           uint32_t *end, uint64_t *cell_row_off)
{
    std::lock_guard<std::mutex> lk(g_kept.mu);
    if (g_kept.row_ptr.empty()) return fail(OEM_ERR_STATE, "oem_debug_cells_records_last_csr: no group was kept (OEM_TEST_KEEP_RECORDS_CSR=1)");
    const size_t nnz = g_kept.tid.size();
    if (dims3) {
        dims3[0] = g_kept.row_ptr.size() - 1;
        dims3[1] = nnz;
        dims3[2] = g_kept.cell_row_off.size() - 1;
    }
    if (row_ptr) std::memcpy(row_ptr, g_kept.row_ptr.data(), sizeof(uint32_t) * g_kept.row_ptr.size());
    if (tid && nnz) std::memcpy(tid, g_kept.tid.data(), sizeof(uint32_t) * nnz);
    if (as_prob_bits && nnz) std::memcpy(as_prob_bits, g_kept.as_prob.data(), sizeof(uint32_t) * nnz);
    if (start && nnz) std::memcpy(start, g_kept.start.data(), sizeof(uint32_t) * nnz);
    if (end && nnz) std::memcpy(end, g_kept.end.data(), sizeof(uint32_t) * nnz);
    if (cell_row_off) std::memcpy(cell_row_off, g_kept.cell_row_off.data(), sizeof(uint64_t) * g_kept.cell_row_off.size());
    return OEM_OK;
}

} // namespace oem

using namespace oem;

extern "C" int oem_em_run_cells_records_sparse(const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                                               const oem_aln_record *records, const uint64_t *group_off, uint64_t n_groups,
                                               const uint64_t *cell_group_off, uint32_t n_cells, uint32_t bin_width, int model,
                                               double growth_rate, int device, uint32_t max_iter, double conv_thresh,
                                               uint32_t *out_kept, oem_cells_result **out)
{
    OEM_API_BEGIN
    const char *who = "oem_em_run_cells_records_sparse";
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    // the checks of oem_store_create_records, of the cells calls and of cell_group_off, before any device use
    OEM_TRY(check_store_from_records(who, filters, txp_len, n_txps, bin_width, model, nullptr));
    RecordsFilter rf;
    std::vector<float> tab_unused;
    bool host_only = false;
    OEM_TRY(filter_prepare_batch(who, *filters, records, group_off, n_groups, &tab_unused, &host_only));
    if (model >= 0) OEM_TRY(check_cells_coverage_args(who, bin_width, model, n_txps, 0, 0));
    OEM_TRY(check_cell_group_off(who, cell_group_off, n_cells, n_groups));
    OEM_TRY(ensure_device(device));
    OEM_TRY(records_filter_setup(who, filters, txp_len, n_txps, &rf));

    CellsCoverage cc;
    CellsRun run{n_txps, device, max_iter, conv_thresh};
    if (model >= 0) { // the per-call part of the coverage model (the annotation), shared by the groups
        cc.txp_len = rf.txp_len.data();
        cc.n_txps = n_txps;
        cc.bin_width = bin_width;
        cc.model = model;
        cc.growth_rate = growth_rate;
        OEM_TRY(cells_coverage_setup(&cc));
        run.cov = &cc;
    }
    std::unique_ptr<oem_cells_result> r(new oem_cells_result());
    r->n_cells = n_cells;
    r->infos.resize(n_cells);
    r->from_records = true;
    r->discard.assign(n_cells, oem_discard_table{});
    const std::vector<std::pair<uint32_t, uint32_t>> groups = cut_cells_groups(cell_group_off, n_cells, group_off, n_txps);
    std::vector<SparseBlock> blocks(groups.size());
    OEM_TRY(run_cells_workers(who, run, groups, [&](size_t g, const CellsRun &grun, CellsGroupPath *path) -> int {
        const uint32_t c0 = groups[g].first, c1 = groups[g].second;
        const uint64_t g0 = cell_group_off[c0], g1 = cell_group_off[c1], r0 = group_off[g0];
        std::vector<uint64_t> goff(g1 - g0 + 1), cgo((size_t)(c1 - c0) + 1); // the group's own offsets, from 0
        for (uint64_t k = 0; k <= g1 - g0; ++k) goff[k] = group_off[g0 + k] - r0;
        for (uint32_t c = c0; c <= c1; ++c) cgo[c - c0] = cell_group_off[c] - g0;
        RecordsGroup rg;
        rg.records = records ? records + r0 : nullptr;
        rg.group_off = goff.data();
        rg.n_groups = g1 - g0;
        rg.cell_group_off = cgo.data();
        rg.n_cells = c1 - c0;
        rg.first_cell = c0;
        rg.first_record = r0;
        rg.out_kept = out_kept ? out_kept + g0 : nullptr;
        rg.out_tables = r->discard.data() + c0;
        rg.blk = &blocks[g];
        rg.infos = r->infos.data() + c0;
        rg.launch = &path->launch;
        bool batched = false;
        const int rc = run_records_group(who, grun, rf, rg, &batched);
        path->batched = batched ? 1u : 0u;
        return rc;
    }));
    OEM_TRY(cells_result_from_blocks(who, blocks, r.get()));
    *out = r.release();
    return OEM_OK;
    OEM_API_END("oem_em_run_cells_records_sparse")
}

extern "C" int oem_em_run_cells_records_names_sparse(const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                                                     const oem_aln_record *records, uint64_t n_records, const uint8_t *names,
                                                     const uint64_t *name_off, const uint8_t *secondary, const uint64_t *cell_rec_off,
                                                     uint32_t n_cells, uint32_t mode, uint32_t bin_width, int model, double growth_rate,
                                                     int device, uint32_t max_iter, double conv_thresh, uint32_t *out_order,
                                                     uint64_t *out_group_off, uint64_t *out_n_groups, uint64_t *out_cell_group_off,
                                                     uint32_t *out_kept, oem_cells_result **out)
{
    OEM_API_BEGIN
    const char *who = "oem_em_run_cells_records_names_sparse";
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (out_n_groups) *out_n_groups = 0;
    // the checks of oem_store_create_records, of oem_collate_names and of the cells calls, before any device use
    OEM_TRY(check_store_from_records(who, filters, txp_len, n_txps, bin_width, model, nullptr));
    if (!name_off || !cell_rec_off) return fail(OEM_ERR_ARG, "%s: name_off or cell_rec_off is NULL", who);
    OEM_TRY(check_collate_input(who, names, name_off, n_records, cell_rec_off, n_cells, mode));
    if (n_records && !records) return fail(OEM_ERR_ARG, "%s: records is NULL", who);
    if (model >= 0) OEM_TRY(check_cells_coverage_args(who, bin_width, model, n_txps, 0, 0));
    OEM_TRY(ensure_device(device));
    RecordsFilter rf;
    OEM_TRY(records_filter_setup(who, filters, txp_len, n_txps, &rf));

    CellsCoverage cc;
    CellsRun run{n_txps, device, max_iter, conv_thresh};
    if (model >= 0) {
        cc.txp_len = rf.txp_len.data();
        cc.n_txps = n_txps;
        cc.bin_width = bin_width;
        cc.model = model;
        cc.growth_rate = growth_rate;
        OEM_TRY(cells_coverage_setup(&cc));
        run.cov = &cc;
    }
    std::unique_ptr<oem_cells_result> r(new oem_cells_result());
    r->n_cells = n_cells;
    r->infos.resize(n_cells);
    r->from_records = true;
    r->discard.assign(n_cells, oem_discard_table{});

    const std::vector<std::pair<uint32_t, uint32_t>> groups =
        cut_names_groups(cell_rec_off, n_cells, n_txps, [&](uint32_t c) { return name_off[cell_rec_off[c]]; });
    NamesCall nc;
    nc.in.who = who;
    nc.in.names = names;
    nc.in.name_off = name_off;
    nc.in.secondary = secondary;
    nc.in.cell_rec_off = cell_rec_off;
    nc.in.mode = mode;
    nc.in.chunk_bytes = collate_chunk_bytes();
    nc.records = records;
    nc.out_order = out_order;
    nc.want_group_off = out_group_off != nullptr;
    nc.want_kept = out_kept != nullptr;
    std::vector<SparseBlock> blocks(groups.size());
    std::vector<NamesSlot> slots(groups.size());
    OEM_TRY(run_cells_workers(who, run, groups, [&](size_t g, const CellsRun &grun, CellsGroupPath *path) -> int {
        const uint32_t c0 = groups[g].first, c1 = groups[g].second;
        RecordsGroup rg;
        rg.out_tables = r->discard.data() + c0;
        rg.blk = &blocks[g];
        rg.infos = r->infos.data() + c0;
        rg.launch = &path->launch;
        bool batched = false;
        const int rc = run_names_group(who, grun, rf, nc, c0, c1, rg, &slots[g], &batched);
        path->batched = batched ? 1u : 0u;
        return rc;
    }));
    names_call_outputs(groups, slots, cell_rec_off, n_records, out_group_off, out_n_groups, out_cell_group_off, out_kept);
    OEM_TRY(cells_result_from_blocks(who, blocks, r.get()));
    *out = r.release();
    return OEM_OK;
    OEM_API_END("oem_em_run_cells_records_names_sparse")
}

// The body of oem_em_run_cells_records_barcodes_sparse and, with_umis, of oem_em_run_cells_records_umis_sparse: the same
// call with the UMIs resident beside the names and every group of cells deduplicated behind its name collation.  UMIs
// that are all empty take no part anywhere: the call is then the barcodes call, and reports no duplicate.
static int cells_records_barcodes_call(const char *who, const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                                       const oem_aln_record *records, uint64_t n_records, const uint8_t *barcodes,
                                       const uint64_t *barcode_off, const uint8_t *names, const uint64_t *name_off,
                                       const uint8_t *secondary, bool with_umis, const oem_umi_rule *rule, const uint8_t *umis,
                                       const uint64_t *umi_off, uint32_t mode,
                                       uint32_t bin_width, int model, double growth_rate, int device, uint32_t max_iter, double conv_thresh,
                                       uint32_t *out_order, uint64_t *out_n_survivors, uint64_t *out_cell_rec_off, uint64_t *out_n_cells,
                                       uint64_t *out_group_off, uint64_t *out_n_groups, uint64_t *out_cell_group_off, uint32_t *out_kept,
                                       uint64_t *out_cell_dups, uint64_t *out_cell_corrected, const oem_barcode_rule *wl_rule,
                                       uint32_t *out_wl_id, uint8_t *out_status, uint64_t *out_counts, oem_cells_result **out)
{
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (out_n_groups) *out_n_groups = 0;
    if (out_n_cells) *out_n_cells = 0;
    if (out_n_survivors) *out_n_survivors = 0;
    // the checks of oem_store_create_records, of oem_collate_barcodes, of oem_collate_names and of the cells calls, before
    // any device use
    OEM_TRY(check_store_from_records(who, filters, txp_len, n_txps, bin_width, model, nullptr));
    if (!barcode_off || !name_off) return fail(OEM_ERR_ARG, "%s: barcode_off or name_off is NULL", who);
    if (wl_rule) OEM_TRY(check_barcode_rule(who, wl_rule));
    OEM_TRY(check_barcode_input(who, barcodes, barcode_off, n_records));
    const uint64_t n = n_records, one_cell[2] = {0, n};
    OEM_TRY(check_collate_input(who, names, name_off, n, one_cell, 1, mode));
    if (n && !records) return fail(OEM_ERR_ARG, "%s: records is NULL", who);
    if (with_umis) {
        if (!umi_off) return fail(OEM_ERR_ARG, "%s: umi_off is NULL", who);
        OEM_TRY(check_offsets(who, "umi_off", umi_off, n, "record"));
        if (umi_off[n] && !umis) return fail(OEM_ERR_ARG, "%s: umis is NULL and the UMIs are not all empty", who);
    }
    const uint32_t *gene_of = rule ? rule->gene_of : nullptr;
    if (rule) {
        if (rule->correct > 1) return fail(OEM_ERR_ARG, "%s: rule->correct = %u is neither 0 nor 1", who, rule->correct);
        if (gene_of && !rule->n_txps) return fail(OEM_ERR_ARG, "%s: rule->gene_of is given and rule->n_txps is 0", who);
        if (gene_of && rule->n_txps != n_txps)
            return fail(OEM_ERR_ARG, "%s: rule->n_txps = %u is not n_txps = %u", who, rule->n_txps, n_txps);
    }
    bool dedup = with_umis && n && umi_off[n] > 0;
    if (model >= 0) OEM_TRY(check_cells_coverage_args(who, bin_width, model, n_txps, 0, 0));
    OEM_TRY(ensure_device(device));
    RecordsFilter rf;
    OEM_TRY(records_filter_setup(who, filters, txp_len, n_txps, &rf));

    CellsCoverage cc;
    CellsRun run{n_txps, device, max_iter, conv_thresh};
    if (model >= 0) {
        cc.txp_len = rf.txp_len.data();
        cc.n_txps = n_txps;
        cc.bin_width = bin_width;
        cc.model = model;
        cc.growth_rate = growth_rate;
        OEM_TRY(cells_coverage_setup(&cc));
        run.cov = &cc;
    }
    const bool timing = knob("OEM_COLLATE_TIMING", 0) != 0;
    double last[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bc_info[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bc_cells_ms = 0;
    std::memset(g_cells_barcodes_last, 0, sizeof g_cells_barcodes_last);

    // the cells: order_bc and cell_rec_off stay on the device, the offsets come down for the cut.  Under a barcode rule
    // they are the cells of the ACCEPTED records: from here on the POSITIONS (na = cro[n_cells], what order_bc holds and
    // every offset counts) and the RECORDS (n, resident in input order and indexed by order_bc's entries) are two numbers.
    BarcodeCells bc;
    std::vector<uint64_t> cro(1, 0), cell_name_off(1, 0);
    uint64_t na = n;
    auto t0 = clk::now();
    if (n && wl_rule) {
        CorrectedCells cor;
        {
            BarcodeWhitelist wl; // released before the records go up
            OEM_TRY(whitelist_build(who, wl_rule, &wl));
            OEM_TRY(correct_barcodes_resident(who, wl, barcodes, barcode_off, n, &cor));
        }
        na = cor.n_accepted;
        std::vector<uint8_t> status;
        if (out_status || dedup) {
            status.resize(n);
            OEM_HIP(hipMemcpy(status.data(), cor.status.p, n, hipMemcpyDeviceToHost));
        }
        if (out_wl_id) OEM_HIP(hipMemcpy(out_wl_id, cor.id.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
        if (out_status) std::copy(status.begin(), status.end(), out_status);
        if (out_counts) std::copy(cor.counts, cor.counts + kBarcodeStatuses, out_counts);
        if (dedup) { // the UMIs of rejected records take no part: accepted UMIs that are all empty deduplicate nothing
            dedup = false;
            for (uint64_t i = 0; i < n && !dedup; ++i) dedup = status[i] <= kBarcodeCorrected && umi_off[i + 1] > umi_off[i];
        }
        std::swap(bc.order.p, cor.cells.order.p);
        std::swap(bc.cell_rec_off.p, cor.cells.cell_rec_off.p);
        bc.n_cells = cor.cells.n_cells;
        if (na) {
            cro.resize(bc.n_cells + 1);
            OEM_HIP(hipMemcpy(cro.data(), bc.cell_rec_off.p, sizeof(uint64_t) * (bc.n_cells + 1), hipMemcpyDeviceToHost));
        }
    } else if (n) {
        OEM_TRY(collate_barcodes_resident(who, barcodes, barcode_off, n, timing, bc_info, &bc_cells_ms, &bc));
        cro.resize(bc.n_cells + 1);
        OEM_HIP(hipMemcpy(cro.data(), bc.cell_rec_off.p, sizeof(uint64_t) * (bc.n_cells + 1), hipMemcpyDeviceToHost));
    } else if (out_counts && wl_rule) {
        std::fill(out_counts, out_counts + kBarcodeStatuses, 0ull);
    }
    bc_info[2] = bc_cells_ms;
    collate_barcodes_set_last(bc_info);
    const uint32_t n_cells = (uint32_t)bc.n_cells;
    last[0] = (double)n_cells;
    last[2] = ms_since(t0);

    // the whole input, once and in input order; the names are checked behind their chunks
    DevBuf<oem_aln_record> d_records;
    DevBuf<uint8_t> d_names, d_sec, d_umis;
    DevBuf<uint64_t> d_name_off, d_gathered_off, d_cell_name_off, d_umi_off;
    t0 = clk::now();
    if (na) {
        const uint64_t n_bytes = name_off[n], chunk_bytes = collate_chunk_bytes();
        DevBuf<unsigned long long> d_bad;
        OEM_TRY(dev_alloc(&d_names.p, n_bytes + 16, nullptr));
        OEM_TRY(dev_alloc(&d_name_off.p, n + 1, nullptr));
        OEM_TRY(dev_alloc(&d_bad.p, 2, nullptr));
        OEM_TRY(dev_alloc(&d_records.p, n, nullptr));
        const unsigned long long bad0[2] = {kNoRecord, kNoRecord};
        OEM_HIP(hipMemcpy(d_bad.p, bad0, sizeof bad0, hipMemcpyHostToDevice));
        OEM_HIP(hipMemcpy(d_name_off.p, name_off, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice));
        OEM_HIP(hipMemset(d_names.p + n_bytes, 0, 16));
        std::vector<uint64_t> byte_cut{0}, rec_cut{0};
        for (uint64_t r = 0; r < n;) {
            uint64_t r1 = (uint64_t)(std::upper_bound(name_off + r + 1, name_off + n + 1, name_off[r] + chunk_bytes) - name_off) - 1;
            r1 = std::max(r1, r + 1);
            byte_cut.push_back(name_off[r1]);
            rec_cut.push_back(r1);
            r = r1;
        }
        float ms[6] = {0, 0, 0, 0, 0, 0};
        OEM_TRY(filter_upload_measure<uint8_t>(names, d_names.p, byte_cut.data(), byte_cut.size() - 1, 1, timing ? ms : nullptr,
                                               [&](hipStream_t lane, uint64_t g0, uint64_t) {
                                                   if (wl_rule) return; // a rejected record's name is never looked at
                                                   launch_collate_validate(lane, d_names.p, byte_cut[g0], byte_cut[g0 + 1], d_name_off.p,
                                                                           rec_cut[g0], rec_cut[g0 + 1], d_bad.p);
                                               }));
        last[6] = ms[0];
        last[7] = ms[1];
        unsigned long long bad[2];
        OEM_HIP(hipMemcpy(bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
        if (wl_rule) OEM_TRY(validate_records_of(bc.order.p, na, d_names.p, d_name_off.p, bad));
        if (bad[0] != kNoRecord || bad[1] != kNoRecord) {
            if (bad[1] < bad[0]) return fail(OEM_ERR_ARG, "%s: record %llu has an empty name", who, bad[1]);
            return fail(OEM_ERR_ARG, "%s: the name of record %llu contains a 0 byte", who, bad[0]);
        }
        if (secondary && mode == kCollateSort) { // (read through aligned 4-byte words: padded)
            OEM_TRY(dev_alloc(&d_sec.p, n + 8, nullptr));
            OEM_HIP(hipMemset(d_sec.p + n, 0, 8));
            OEM_HIP(hipMemcpy(d_sec.p, secondary, n, hipMemcpyHostToDevice));
        }
        if (dedup) OEM_TRY(umis_upload(who, umis, umi_off, n, &d_umis, &d_umi_off, wl_rule == nullptr));
        if (dedup && wl_rule) { // ... nor is its UMI
            unsigned long long bad_umi[2];
            OEM_TRY(validate_records_of(bc.order.p, na, d_umis.p, d_umi_off.p, bad_umi));
            if (bad_umi[0] != kNoRecord) return fail(OEM_ERR_ARG, "%s: the UMI of record %llu contains a 0 byte", who, bad_umi[0]);
        }
        OEM_TRY(upload_records(records, n, d_records.p));
        last[3] = ms_since(t0);
        t0 = clk::now();
        OEM_TRY(dev_alloc(&d_gathered_off.p, na + 1, nullptr));
        OEM_TRY(gather_name_offsets(bc.order.p, na, d_name_off.p, d_gathered_off.p));
        OEM_TRY(dev_alloc(&d_cell_name_off.p, (size_t)n_cells + 1, nullptr));
        hipLaunchKernelGGL(k_sample_offsets, dim3((n_cells + 1 + kGT - 1) / kGT), dim3(kGT), 0, nullptr, (uint64_t)n_cells + 1,
                           (const uint64_t *)bc.cell_rec_off.p, (const uint64_t *)d_gathered_off.p, d_cell_name_off.p);
        OEM_HIP(hipGetLastError());
        cell_name_off.resize((size_t)n_cells + 1);
        OEM_HIP(hipMemcpy(cell_name_off.data(), d_cell_name_off.p, sizeof(uint64_t) * ((size_t)n_cells + 1), hipMemcpyDeviceToHost));
        d_cell_name_off.reset();
        last[4] = ms_since(t0);
    }

    std::unique_ptr<oem_cells_result> r(new oem_cells_result());
    r->n_cells = n_cells;
    r->infos.resize(n_cells);
    r->from_records = true;
    r->discard.assign(n_cells, oem_discard_table{});
    const std::vector<std::pair<uint32_t, uint32_t>> groups =
        cut_names_groups(cro.data(), n_cells, n_txps, [&](uint32_t c) { return cell_name_off[c]; });
    ResidentInput dv;
    dv.records = d_records.p;
    dv.names = d_names.p;
    dv.sec = d_sec.p;
    dv.name_off = d_name_off.p;
    dv.order_bc = bc.order.p;
    dv.gathered_off = d_gathered_off.p;
    dv.cell_name_off = cell_name_off.data();
    UmiInput um; // the flags are read where they are: word 8 of a record's ten
    static_assert(offsetof(oem_aln_record, flags) == 32 && sizeof(oem_aln_record) == 40, "the flags word of a resident record");
    um.who = who;
    um.d_umis = d_umis.p;
    um.d_umi_off = d_umi_off.p;
    um.d_flags = d_records.p ? (const uint32_t *)d_records.p + 8 : nullptr;
    um.flags_stride = 10;
    DevBuf<uint32_t> d_gene_of;
    if (dedup && gene_of) { // ... and so is the ref_id: word 0
        static_assert(offsetof(oem_aln_record, ref_id) == 0, "the ref_id word of a resident record");
        OEM_TRY(dev_alloc(&d_gene_of.p, n_txps, nullptr));
        OEM_HIP(hipMemcpy(d_gene_of.p, gene_of, sizeof(uint32_t) * n_txps, hipMemcpyHostToDevice));
        um.d_ref_id = (const uint32_t *)d_records.p;
        um.ref_id_stride = 10;
        um.d_gene_of = d_gene_of.p;
        um.n_txps = n_txps;
    }
    um.correct = rule ? rule->correct : 0u;
    if (rule) dedup_rule_reset_last();
    if (dedup) dv.umi = &um;
    NamesCall nc;
    nc.in.who = who;
    nc.in.cell_rec_off = cro.data();
    nc.in.mode = mode;
    nc.in.chunk_bytes = collate_chunk_bytes();
    nc.dev = &dv;
    nc.records = records;
    nc.out_order = out_order;
    nc.want_group_off = out_group_off != nullptr;
    nc.want_kept = out_kept != nullptr;
    std::vector<SparseBlock> blocks(groups.size());
    std::vector<NamesSlot> slots(groups.size());
    t0 = clk::now();
    OEM_TRY(run_cells_workers(who, run, groups, [&](size_t g, const CellsRun &grun, CellsGroupPath *path) -> int {
        const uint32_t c0 = groups[g].first, c1 = groups[g].second;
        RecordsGroup rg;
        rg.out_tables = r->discard.data() + c0;
        rg.blk = &blocks[g];
        rg.infos = r->infos.data() + c0;
        rg.launch = &path->launch;
        bool batched = false;
        const int rc = run_names_group(who, grun, rf, nc, c0, c1, rg, &slots[g], &batched);
        path->batched = batched ? 1u : 0u;
        return rc;
    }));
    last[1] = (double)groups.size();
    last[5] = ms_since(t0);
    if (dedup) {
        umis_call_outputs(groups, slots, out_order, out_n_survivors, out_cell_rec_off, out_group_off, out_n_groups, out_cell_group_off, out_kept,
                          out_cell_dups, out_cell_corrected);
    } else {
        names_call_outputs(groups, slots, cro.data(), na, out_group_off, out_n_groups, out_cell_group_off, out_kept);
        if (out_cell_rec_off) std::memcpy(out_cell_rec_off, cro.data(), sizeof(uint64_t) * ((size_t)n_cells + 1));
        if (out_n_survivors) *out_n_survivors = na;
        if (out_cell_dups) std::fill(out_cell_dups, out_cell_dups + n_cells, 0ull);
        if (out_cell_corrected) std::fill(out_cell_corrected, out_cell_corrected + n_cells, 0ull);
    }
    OEM_TRY(cells_result_from_blocks(who, blocks, r.get()));
    if (out_n_cells) *out_n_cells = n_cells;
    std::memcpy(g_cells_barcodes_last, last, sizeof last);
    *out = r.release();
    return OEM_OK;
}

extern "C" int oem_em_run_cells_records_barcodes_sparse(const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                                                        const oem_aln_record *records, uint64_t n_records, const uint8_t *barcodes,
                                                        const uint64_t *barcode_off, const uint8_t *names, const uint64_t *name_off,
                                                        const uint8_t *secondary, uint32_t mode, uint32_t bin_width, int model,
                                                        double growth_rate, int device, uint32_t max_iter, double conv_thresh,
                                                        uint32_t *out_order, uint64_t *out_cell_rec_off, uint64_t *out_n_cells,
                                                        uint64_t *out_group_off, uint64_t *out_n_groups, uint64_t *out_cell_group_off,
                                                        uint32_t *out_kept, oem_cells_result **out)
{
    OEM_API_BEGIN
    return cells_records_barcodes_call("oem_em_run_cells_records_barcodes_sparse", filters, txp_len, n_txps, records, n_records, barcodes,
                                       barcode_off, names, name_off, secondary, false, nullptr, nullptr, nullptr, mode, bin_width, model, growth_rate,
                                       device, max_iter, conv_thresh, out_order, nullptr, out_cell_rec_off, out_n_cells, out_group_off,
                                       out_n_groups, out_cell_group_off, out_kept, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out);
    OEM_API_END("oem_em_run_cells_records_barcodes_sparse")
}

extern "C" int oem_em_run_cells_records_umis_sparse(const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                                                    const oem_aln_record *records, uint64_t n_records, const uint8_t *barcodes,
                                                    const uint64_t *barcode_off, const uint8_t *names, const uint64_t *name_off,
                                                    const uint8_t *secondary, const uint8_t *umis, const uint64_t *umi_off, uint32_t mode,
                                                    uint32_t bin_width, int model, double growth_rate, int device, uint32_t max_iter,
                                                    double conv_thresh, uint32_t *out_order, uint64_t *out_n_survivors,
                                                    uint64_t *out_cell_rec_off, uint64_t *out_n_cells, uint64_t *out_group_off,
                                                    uint64_t *out_n_groups, uint64_t *out_cell_group_off, uint32_t *out_kept,
                                                    uint64_t *out_cell_dups, oem_cells_result **out)
{
    OEM_API_BEGIN
    return cells_records_barcodes_call("oem_em_run_cells_records_umis_sparse", filters, txp_len, n_txps, records, n_records, barcodes,
                                       barcode_off, names, name_off, secondary, true, nullptr, umis, umi_off, mode, bin_width, model, growth_rate,
                                       device, max_iter, conv_thresh, out_order, out_n_survivors, out_cell_rec_off, out_n_cells, out_group_off,
                                       out_n_groups, out_cell_group_off, out_kept, out_cell_dups, nullptr, nullptr, nullptr, nullptr, nullptr, out);
    OEM_API_END("oem_em_run_cells_records_umis_sparse")
}

extern "C" int oem_em_run_cells_records_umis_rule_sparse(const oem_umi_rule *rule, const oem_filters *filters, const uint64_t *txp_len,
                                                         uint32_t n_txps, const oem_aln_record *records, uint64_t n_records,
                                                         const uint8_t *barcodes, const uint64_t *barcode_off, const uint8_t *names,
                                                         const uint64_t *name_off, const uint8_t *secondary, const uint8_t *umis,
                                                         const uint64_t *umi_off, uint32_t mode, uint32_t bin_width, int model,
                                                         double growth_rate, int device, uint32_t max_iter, double conv_thresh,
                                                         uint32_t *out_order, uint64_t *out_n_survivors, uint64_t *out_cell_rec_off,
                                                         uint64_t *out_n_cells, uint64_t *out_group_off, uint64_t *out_n_groups,
                                                         uint64_t *out_cell_group_off, uint32_t *out_kept, uint64_t *out_cell_dups,
                                                         uint64_t *out_cell_corrected, oem_cells_result **out)
{
    OEM_API_BEGIN
    return cells_records_barcodes_call("oem_em_run_cells_records_umis_rule_sparse", filters, txp_len, n_txps, records, n_records, barcodes,
                                       barcode_off, names, name_off, secondary, true, rule, umis, umi_off, mode, bin_width, model, growth_rate,
                                       device, max_iter, conv_thresh, out_order, out_n_survivors, out_cell_rec_off, out_n_cells, out_group_off,
                                       out_n_groups, out_cell_group_off, out_kept, out_cell_dups, out_cell_corrected, nullptr, nullptr, nullptr, nullptr, out);
    OEM_API_END("oem_em_run_cells_records_umis_rule_sparse")
}

extern "C" int oem_em_run_cells_records_whitelist_sparse(const oem_barcode_rule *rule, const oem_umi_rule *umi_rule, const oem_filters *filters,
                                                         const uint64_t *txp_len, uint32_t n_txps, const oem_aln_record *records,
                                                         uint64_t n_records, const uint8_t *barcodes, const uint64_t *barcode_off,
                                                         const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary,
                                                         const uint8_t *umis, const uint64_t *umi_off, uint32_t mode, uint32_t bin_width,
                                                         int model, double growth_rate, int device, uint32_t max_iter, double conv_thresh,
                                                         uint32_t *out_order, uint64_t *out_n_survivors, uint64_t *out_cell_rec_off,
                                                         uint64_t *out_n_cells, uint64_t *out_group_off, uint64_t *out_n_groups,
                                                         uint64_t *out_cell_group_off, uint32_t *out_kept, uint64_t *out_cell_dups,
                                                         uint64_t *out_cell_corrected, uint32_t *out_wl_id, uint8_t *out_status,
                                                         uint64_t *out_counts, oem_cells_result **out)
{
    OEM_API_BEGIN
    const char *who = "oem_em_run_cells_records_whitelist_sparse";
    if (out) *out = nullptr;
    if (!rule) return fail(OEM_ERR_ARG, "%s: the barcode rule is NULL", who);
    if (umis && !umi_off) return fail(OEM_ERR_ARG, "%s: umis is given and umi_off is NULL", who);
    return cells_records_barcodes_call(who, filters, txp_len, n_txps, records, n_records, barcodes, barcode_off, names, name_off, secondary,
                                       umi_off != nullptr, umi_rule, umis, umi_off, mode, bin_width, model, growth_rate, device, max_iter,
                                       conv_thresh, out_order, out_n_survivors, out_cell_rec_off, out_n_cells, out_group_off, out_n_groups,
                                       out_cell_group_off, out_kept, out_cell_dups, out_cell_corrected, rule, out_wl_id, out_status, out_counts,
                                       out);
    OEM_API_END("oem_em_run_cells_records_whitelist_sparse")
}

extern "C" int oem_cells_result_discard_tables(const oem_cells_result *r, oem_discard_table *out)
{
    if (!r || !out) return fail(OEM_ERR_ARG, "oem_cells_result_discard_tables: NULL argument");
    if (!r->from_records) return fail(OEM_ERR_STATE, "oem_cells_result_discard_tables: the result did not come from records");
    if (!r->discard.empty()) std::memcpy(out, r->discard.data(), sizeof(oem_discard_table) * r->discard.size());
    return OEM_OK;
}
