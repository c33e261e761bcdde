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
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "oem_cells.h"
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

} // namespace

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
    const int rc = run_cells_group(run, cg, batched);
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

extern "C" int oem_cells_result_discard_tables(const oem_cells_result *r, oem_discard_table *out)
{
    if (!r || !out) return fail(OEM_ERR_ARG, "oem_cells_result_discard_tables: NULL argument");
    if (!r->from_records) return fail(OEM_ERR_STATE, "oem_cells_result_discard_tables: the result did not come from records");
    if (!r->discard.empty()) std::memcpy(out, r->discard.data(), sizeof(oem_discard_table) * r->discard.size());
    return OEM_OK;
}
