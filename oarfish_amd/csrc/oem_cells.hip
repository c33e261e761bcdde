// oem_cells.hip -- single_cell.rs:139-160: an independent em::em per cell.  All cells of a group are laid out as
// ONE store over a concatenated transcript space and share every pass (oem_multi_kernels.hip); groups the tiler
// declines run cell after cell over the caller-order CSR.
#include <algorithm>
#include <atomic>
#include <functional>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "oem_cells.h"

namespace oem {

#ifndef OEM_CELLS_HEAD_DIV
#define OEM_CELLS_HEAD_DIV 4 // a large single group is split head : rest = 1 : (div - 1); 0 = not split
#endif

// ---- helpers
// The EM loops of the groups of one call (they may run on two host threads and add themselves under the lock); the
// calling thread copies the result into its thread-local pair at the end, for oem_cells_last_timing.
struct CellsTiming {
    std::mutex mu;
    std::vector<std::pair<double, double>> loops; // [begin, end) of every group's EM loop, ms on the host's steady clock
    uint64_t passes = 0;
    // Time during which at least one group's loop ran: groups of one call overlap on the device (two workers), and
    // the sum of their durations would count the shared time twice.
    double loop_ms()
    {
        std::sort(loops.begin(), loops.end());
        double total = 0.0, cur_b = 0.0, cur_e = -1.0;
        for (const auto &iv : loops) {
            if (cur_e < cur_b || iv.first > cur_e) {
                if (cur_e > cur_b) total += cur_e - cur_b;
                cur_b = iv.first;
                cur_e = iv.second;
            } else if (iv.second > cur_e) {
                cur_e = iv.second;
            }
        }
        if (cur_e > cur_b) total += cur_e - cur_b;
        return total;
    }
};

namespace {

constexpr uint32_t kCellsHeadDiv = OEM_CELLS_HEAD_DIV;

// What the last oem_em_run_cells call of this thread spent in its batched EM loops (HIP events on the
// group's stream around the loop), for oem_cells_last_timing.
thread_local double t_cells_loop_ms = 0.0;
thread_local uint64_t t_cells_batched_passes = 0;
// The groups of the last per-cell call of this thread and the path each one took, for oem_debug_cells_last_paths.
thread_local std::vector<CellsGroupPath> t_cells_paths;

// Device buffers of the count / scan / emit steps, kept across the cells of a cell-by-cell group.
struct NzScratch {
    DevBuf<uint32_t> counts, col;
    DevBuf<uint64_t> off;
    DevBuf<float> val;
    size_t cap_cells = 0, cap_entries = 0;
};

struct EventPair { // the HIP events around a group's EM loop
    hipEvent_t begin = nullptr, end = nullptr;
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair()
    {
        if (begin) hipEventDestroy(begin);
        if (end) hipEventDestroy(end);
    }
};

struct StoreFree {
    void operator()(oem_store *s) const { free_store(s); }
};
using StorePtr = std::unique_ptr<oem_store, StoreFree>;

// ---- sinks
// single_cell.rs:151-160 on the device: the entries > 0.0 of cells [0, n_cells) of `src`, in ascending transcript id,
// appended to `blk` (k_cells_nz_count, a host scan of the counts, k_cells_nz_emit, then only the entries cross PCIe).
// cell_aln_off: the cells' first alignments -- a cell cannot have more entries than alignments.
int cells_to_csr(hipStream_t st, const CellsNzSource &src, uint32_t n_cells, const uint64_t *cell_aln_off, NzScratch &sc,
                 SparseBlock *blk)
{
    if (n_cells == 0) return OEM_OK;
    if (n_cells > sc.cap_cells) {
        sc.counts.reset();
        sc.off.reset();
        sc.cap_cells = 0;
        OEM_TRY(dev_alloc(&sc.counts.p, n_cells, nullptr));
        OEM_TRY(dev_alloc(&sc.off.p, (size_t)n_cells + 1, nullptr));
        sc.cap_cells = n_cells;
    }
    const size_t first = blk->counts.size();
    blk->counts.resize(first + n_cells);
    uint32_t *h_counts = blk->counts.data() + first;
    OEM_TRY(launch_cells_nz_count(st, src, n_cells, sc.counts.p));
    OEM_HIP(hipMemcpyAsync(h_counts, sc.counts.p, sizeof(uint32_t) * n_cells, hipMemcpyDeviceToHost, st));
    OEM_HIP(hipStreamSynchronize(st));
    std::vector<uint64_t> off((size_t)n_cells + 1);
    off[0] = 0;
    for (uint32_t c = 0; c < n_cells; ++c) {
        const uint64_t aligned = cell_aln_off[c + 1] - cell_aln_off[c];
        if (h_counts[c] > src.T || h_counts[c] > aligned)
            return fail(OEM_ERR_STATE, "oem_em_run_cells_sparse: cell %u has %u entries, more than its %llu alignments or %u transcripts",
                        c, h_counts[c], (unsigned long long)aligned, src.T);
        off[c + 1] = off[c] + h_counts[c];
    }
    const uint64_t total = off[n_cells];
    const size_t e0 = blk->col.size();
    blk->col.resize(e0 + total);
    blk->val.resize(e0 + total);
    if (total == 0) return OEM_OK;
    if (total > sc.cap_entries) {
        sc.col.reset();
        sc.val.reset();
        sc.cap_entries = 0;
        OEM_TRY(dev_alloc(&sc.col.p, total, nullptr));
        OEM_TRY(dev_alloc(&sc.val.p, total, nullptr));
        sc.cap_entries = total;
    }
    OEM_HIP(hipMemcpyAsync(sc.off.p, off.data(), sizeof(uint64_t) * (n_cells + 1), hipMemcpyHostToDevice, st));
    int rc = launch_cells_nz_emit(st, src, n_cells, sc.off.p, sc.col.p, sc.val.p);
    if (rc == OEM_OK &&
        (hipMemcpyAsync(blk->col.data() + e0, sc.col.p, sizeof(uint32_t) * total, hipMemcpyDeviceToHost, st) != hipSuccess ||
         hipMemcpyAsync(blk->val.data() + e0, sc.val.p, sizeof(float) * total, hipMemcpyDeviceToHost, st) != hipSuccess))
        rc = fail(OEM_ERR_HIP, "oem_em_run_cells_sparse: read-back of the entries failed");
    // (also on failure: `off` must outlive the upload queued above)
    if (hipStreamSynchronize(st) != hipSuccess && rc == OEM_OK) rc = fail(OEM_ERR_HIP, "oem_em_run_cells_sparse: emit failed");
    return rc;
}

// The dense sink of a batched group: its results in the caller's [cell][transcript] rows.  A compacted batch is
// expanded on the device, or on the host when there is no device memory for the expanded results.
int cells_to_dense(oem_store *s, uint32_t n_cells, uint32_t n_txps, double *out)
{
    MultiBuffers &mb = s->multi;
    const uint64_t full_total = (uint64_t)n_cells * n_txps;
    const double *d_res = mb.out;
    DevBuf<double> d_full;
    if (mb.rank) { // compacted
        if (knob("OEM_TEST_FAIL_FULL_ALLOC", 0) || hipMalloc((void **)&d_full.p, sizeof(double) * full_total) != hipSuccess) {
            // the compact results and the rank table go to the host, which expands them (a transcript that does not
            // occur in a cell is 0)
            (void)hipGetLastError();
            d_full.p = nullptr;
            const size_t n_eff = (size_t)mb.n_problems * mb.txps_eff;
            std::vector<double> h_eff(n_eff);
            std::vector<uint32_t> h_rank((size_t)full_total);
            if (hipMemcpy(h_eff.data(), mb.out, sizeof(double) * n_eff, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(h_rank.data(), mb.rank, sizeof(uint32_t) * full_total, hipMemcpyDeviceToHost) != hipSuccess)
                return fail(OEM_ERR_HIP, "oem_em_run_cells: read-back failed");
            for (size_t i = 0; i < (size_t)full_total; ++i)
                out[i] = h_rank[i] == kNoRank ? 0.0 : h_eff[(i / mb.txps_full) * mb.txps_eff + h_rank[i]];
            return OEM_OK;
        }
        // expand to the caller's [cell][transcript] (the queue is done with: its memory is free by now)
        OEM_TRY(launch_multi_expand(s, mb, d_full.p));
        if (hipStreamSynchronize(s->stream) != hipSuccess) return fail(OEM_ERR_HIP, "oem_em_run_cells: expanding the results failed");
        d_res = d_full.p;
    }
    if (hipMemcpy(out, d_res, sizeof(double) * full_total, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(OEM_ERR_HIP, "oem_em_run_cells: result read-back failed");
    return OEM_OK;
}

// ---- the batched run: all cells of a group in one store over the concatenated transcript space; every pass serves
// every unfinished cell.  Three steps: the store, the loop, the read-back.

// Step 1.  *out stays empty when the tiler declines the batch (e.g. a read with > 255 alignments inside one window):
// the cell-by-cell path takes the group, over the resident CSR if there is one.
int create_batched_store(const CellsRun &run, const CellsGroup &g, StorePtr *out)
{
    StorePtr s(new (std::nothrow) oem_store());
    if (!s) return fail(OEM_ERR_OOM, "oem_em_run_cells: host allocation failed");
    oem_store_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.reorder_rows = 0; // a batch that cannot be tiled falls through to the cell-by-cell path
    opts.problem_size = run.n_txps;
    // transcripts of cell p -> [p*T, (p+1)*T), relabelled on the device after the upload
    CellRelabel rl{g.cell_row_off, g.n_cells, run.n_txps, g.d_cell_row_off};
    OEM_TRY(create_store_impl(g.row_ptr, g.tid, g.as_prob, g.cov_prob, g.n_reads, g.nnz, g.n_cells * run.n_txps, run.device, &opts,
                              s.get(), &rl, g.resident));
    if (!s->tiled.present) // the CSR goes back with the caller's ids (they were relabelled)
        return g.resident ? release_resident_csr(s.get(), g.resident, g.tid, g.d_tid_orig) : OEM_OK;
    *out = std::move(s);
    return OEM_OK;
}

// Step 2: the per-cell state, then passes in chunks until every cell has finished.  d_reads (the cells' read counts)
// stays with the caller until the results are back.
int run_batched_loop(const CellsRun &run, const CellsGroup &g, oem_store *s, DevBuf<uint64_t> &d_reads)
{
    const uint32_t n_cells = g.n_cells;
    MultiBuffers &mb = s->multi;
    // transcripts per cell IN THE STORE: the ones that occur in the cell, padded to the fullest cell's count
    // (oem_api.hip: k_cells_mark); the caller's n_txps where the batch was not compacted
    const uint32_t n_txps = mb.rank ? mb.txps_eff : run.n_txps;
    const uint64_t store_total = (uint64_t)n_cells * n_txps;
    mb.n_problems = n_cells;
    mb.problem_size = n_txps;
    OEM_TRY(dev_alloc(&mb.state, n_cells, &s->hbm_bytes));
    OEM_TRY(dev_alloc(&mb.out, (size_t)store_total, &s->hbm_bytes));
    OEM_TRY(dev_alloc(&mb.n_unfinished, 1, &s->hbm_bytes));
    std::vector<BatchState> hs(n_cells);
    std::vector<uint64_t> reads(n_cells);
    for (uint32_t c = 0; c < n_cells; ++c) {
        std::memset(&hs[c], 0, sizeof(BatchState));
        hs[c].phase = kPhaseRunning;
        reads[c] = g.cell_row_off[c + 1] - g.cell_row_off[c]; // the cell's own store.len() (single_cell.rs:122-130)
    }
    OEM_TRY(dev_alloc(&d_reads.p, n_cells, nullptr));
    if (hipMemcpyAsync(d_reads.p, reads.data(), sizeof(uint64_t) * n_cells, hipMemcpyHostToDevice, s->stream) != hipSuccess ||
        hipMemcpyAsync(mb.state, hs.data(), sizeof(BatchState) * n_cells, hipMemcpyHostToDevice, s->stream) != hipSuccess ||
        hipMemcpyAsync(mb.n_unfinished, &n_cells, sizeof(uint32_t), hipMemcpyHostToDevice, s->stream) != hipSuccess ||
        hipMemsetAsync(s->cnt, 0, sizeof(double) * store_total, s->stream) != hipSuccess)
        return fail(OEM_ERR_HIP, "oem_em_run_cells: upload of the per-cell state failed");
    OEM_TRY(launch_multi_init(s, s->theta, d_reads.p, mb));
    EmParams p{n_txps, run.max_iter, 50u /* em::em, single_cell.rs:150 */, run.conv_thresh};
    if (hipMemsetAsync(mb.out, 0, sizeof(double) * store_total, s->stream) != hipSuccess)
        return fail(OEM_ERR_HIP, "oem_em_run_cells: clearing the result buffer failed");
    const uint64_t total = (uint64_t)run.max_iter + 1; // loop passes + the final one (em.rs:245-252)
    // one workgroup per bucket folds the queue AND finishes the pass (k_multi_fold_reldiff); a
    // store without remote alignments has no buckets to own and takes the separate kernels
    const bool fused_fold = s->tiled.n_remote > 0 && s->tiled.n_buckets > 0 && knob("OEM_CELLS_FUSED_FOLD", 1) != 0;
    uint64_t launched = 0;
    uint32_t unfinished = n_cells, compacted_at = n_cells;
    EventPair ev;
    if (hipEventCreate(&ev.begin) != hipSuccess || hipEventCreate(&ev.end) != hipSuccess ||
        hipEventRecord(ev.begin, s->stream) != hipSuccess)
        return fail(OEM_ERR_HIP, "oem_em_run_cells: event set-up failed");
    auto one_pass = [&]() -> int {
        if (fused_fold) {
            OEM_TRY(launch_em_pass_tiled(s, s->theta, s->cnt, nullptr, nullptr, mb.state, n_txps, true));
            return launch_multi_fold_reldiff(s, s->theta, s->cnt, mb, p);
        }
        OEM_TRY(launch_em_pass_tiled(s, s->theta, s->cnt, nullptr, nullptr, mb.state, n_txps));
        return launch_multi_reldiff(s, s->theta, s->cnt, mb, p);
    };
    ChunkGraph cg; // kGraphIters batched passes (five to six kernels each), replayed
    if (graph_ok(s) && total >= 4 * kGraphIters) OEM_TRY(capture_chunk(s->stream, kGraphIters, one_pass, &cg));
    while (launched < total && unfinished) {
        uint64_t chunk = launched == 0 ? 53 : 16;
        if (chunk > total - launched) chunk = total - launched;
        if (cg.ready()) { // (passes beyond `total` find every cell FINISHED: no-ops)
            chunk = (chunk + kGraphIters - 1) / kGraphIters * kGraphIters;
            for (uint64_t k = 0; k < chunk; k += kGraphIters)
                if (hipGraphLaunch(cg.ge, s->stream) != hipSuccess) return fail(OEM_ERR_HIP, "oem_em_run_cells: graph launch failed");
        } else {
            for (uint64_t k = 0; k < chunk; ++k) OEM_TRY(one_pass());
        }
        launched += chunk;
        if (hipMemcpyAsync(&unfinished, mb.n_unfinished, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
            hipStreamSynchronize(s->stream) != hipSuccess)
            return fail(OEM_ERR_HIP, "oem_em_run_cells: state read-back failed");
        // cells have finished since the live lists were built: the next passes launch the live tiles and
        // buckets only (the lists stay supersets of the live work until the next look)
        if (unfinished && unfinished < compacted_at && !cg.ready() && knob("OEM_CELLS_COMPACT", 1) != 0) {
            OEM_TRY(multi_compact_live(s, mb));
            compacted_at = unfinished;
        }
    }
    float ms = 0.f;
    if (hipEventRecord(ev.end, s->stream) == hipSuccess && hipEventSynchronize(ev.end) == hipSuccess &&
        hipEventElapsedTime(&ms, ev.begin, ev.end) == hipSuccess && run.timing) {
        // the loop ended just now and lasted `ms` on the device
        const double end = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
        std::lock_guard<std::mutex> lk(run.timing->mu);
        run.timing->loops.emplace_back(end - (double)ms, end);
        run.timing->passes += launched;
    }
    return OEM_OK;
}

// Step 3: the results through the group's sink, then every cell's final state into `infos`.
int read_back_batched(const CellsRun &run, const CellsGroup &g, oem_store *s)
{
    MultiBuffers &mb = s->multi;
    NzScratch sc;
    if (g.blk) // the entries > 0 straight from the compact (or uncompacted) results: no expansion, no dense copy
        OEM_TRY(cells_to_csr(s->stream, CellsNzSource{mb.out, mb.rank, run.n_txps, mb.problem_size}, g.n_cells, g.cell_aln_off, sc, g.blk));
    else
        OEM_TRY(cells_to_dense(s, g.n_cells, run.n_txps, g.out_dense));
    std::vector<BatchState> hs(g.n_cells);
    if (hipMemcpy(hs.data(), mb.state, sizeof(BatchState) * g.n_cells, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(OEM_ERR_HIP, g.blk ? "oem_em_run_cells_sparse: state read-back failed" : "oem_em_run_cells: result read-back failed");
    if (g.infos)
        for (uint32_t c = 0; c < g.n_cells; ++c) g.infos[c] = run_info_from(hs[c], 0); // (a cell counts its own final pass)
    return OEM_OK;
}

// Returns *used = false (nothing done) when the batch form does not apply.
int run_cells_batched(const CellsRun &run, const CellsGroup &g, bool *used)
{
    *used = false;
    StageTimer tm;
    const uint64_t total_txps = (uint64_t)g.n_cells * run.n_txps;
    if (run.max_iter < 1 || g.n_cells < 2 || total_txps >= (1ull << 32) || g.n_reads >= (1ull << 32)) return OEM_OK;
    tm.lap("cells: group set-up");   // (the arrays were range-checked once by oem_em_run_cells)
    OEM_TRY(ensure_device(run.device));
    StorePtr s;
    OEM_TRY(create_batched_store(run, g, &s));
    if (!s) return OEM_OK;
    *used = true;
    tm.lap("cells: store create");
    if (tm.on)
        fprintf(stderr, "[oem] cells: %u transcripts per cell in the store (of %u), %u tiles, %llu local + %llu remote alignments\n",
                s->multi.rank ? s->multi.txps_eff : run.n_txps, run.n_txps, s->tiled.n_tiles, (unsigned long long)s->tiled.n_local,
                (unsigned long long)s->tiled.n_remote);
    DevBuf<uint64_t> d_reads;
    int rc = run_batched_loop(run, g, s.get(), d_reads);
    if (g.launch) *g.launch = s->last_launch;
    if (rc == OEM_OK) {
        tm.lap("cells: EM loop");
        rc = read_back_batched(run, g, s.get());
    }
    d_reads.reset();
    tm.lap("cells: read-back");
    s.reset();
    tm.lap("cells: free");
    return rc;
}

// The fallback (max_iter == 0, a single cell, or a group the tiler declines): cells one after another, as row ranges
// of one store over the caller-order CSR.
int run_cells_serial(const CellsRun &run, const CellsGroup &g)
{
    oem_store *raw = nullptr;
    oem_store_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.reorder_rows = 1; // cells are row ranges of the caller-order CSR
    NzScratch sc;
    StorePtr s;
    if (g.resident) { // (the arrays were checked by the entry point; the store takes the resident CSR over)
        OEM_TRY(ensure_device(run.device));
        s.reset(new (std::nothrow) oem_store());
        if (!s) return fail(OEM_ERR_OOM, "oem_em_run_cells: host allocation failed");
        OEM_TRY(create_store_impl(g.row_ptr, g.tid, g.as_prob, nullptr, g.n_reads, g.nnz, run.n_txps, run.device, &opts, s.get(),
                                  nullptr, g.resident));
    } else {
        OEM_TRY(oem_store_create(g.row_ptr, g.tid, g.as_prob, g.cov_prob, g.n_reads, g.nnz, run.n_txps, run.device, &opts, &raw));
        s.reset(raw);
    }
    CellsNzSource src; // the cell's count vector (s->cnt after the run, as copy_counts_out reads it), caller's transcript order
    src.T = src.stride = run.n_txps;
    for (uint32_t c = 0; c < g.n_cells; ++c) {
        RunArgs a;
        a.row_begin = g.cell_row_off[c];
        a.row_end = g.cell_row_off[c + 1];
        a.total_reads = a.row_end - a.row_begin; // the cell's own store.len() (single_cell.rs:122-130)
        a.max_iter = run.max_iter;
        a.conv_thresh = run.conv_thresh;
        a.min_iter_gate = 50;                    // em::em (single_cell.rs:150)
        OEM_TRY(run_em_device(s.get(), a, g.infos ? &g.infos[c] : nullptr));
        src.v = s->cnt;
        if (g.blk) OEM_TRY(cells_to_csr(s->stream, src, 1, g.cell_aln_off + c, sc, g.blk));
        else OEM_TRY(copy_counts_out(s.get(), g.out_dense + (uint64_t)c * run.n_txps));
    }
    return OEM_OK;
}

} // namespace

// ---- one group
int run_cells_group(const CellsRun &run, const CellsGroup &g, bool *batched)
{
    *batched = false;
    if (run.cov) { // the coverage model of the group's cells, computed on the device: the weights stay there for the store
        OEM_TRY(ensure_device(run.device));
        OEM_TRY(cells_coverage_group(*run.cov, g, g.resident));
    }
    if (knob("OEM_SERIAL_CELLS", 0) == 0) { // testing build: force the cell-by-cell path
        const int rc = run_cells_batched(run, g, batched);
        if (rc != OEM_OK || *batched) return rc;
    }
    return run_cells_serial(run, g);
}

// ---- the grouping rule
uint64_t cells_max_group_nnz() { return (uint64_t)knob("OEM_CELLS_GROUP_NNZ", 1l << 30); } // testing build: small groups

bool cells_group_fits(uint64_t cells, uint64_t reads, uint64_t gnnz, uint32_t n_txps, uint64_t max_group_nnz)
{
    const uint64_t buckets = (cells * n_txps + kBucket - 1) / kBucket;
    // tiles per group: ~300 reads per tile with the narrow window cap on sparse cells, ~700 with the
    // wide one that create_store_impl picks below 4 reads per transcript
    const bool wide = reads < 2 * cells * n_txps && reads >= 1000000; // as create_store_impl chooses
    const uint64_t tiles_est = reads / (wide ? 600 : 256) + 2 * cells;
    return !(cells * n_txps >= (1ull << 32) || reads >= (1ull << 32) || gnnz > max_group_nnz ||
             tiles_est * buckets > (1ull << 29) || cells > 65535 /* gridDim.y of the per-cell kernels */);
}

// ---- the record of the last call of this thread, and the argument check shared with the coverage entry point
void cells_last_timing(double *loop_ms, uint64_t *batched_passes)
{
    if (loop_ms) *loop_ms = t_cells_loop_ms;
    if (batched_passes) *batched_passes = t_cells_batched_passes;
}

const std::vector<CellsGroupPath> &cells_last_paths() { return t_cells_paths; }

int check_cell_row_off(const char *who, const uint64_t *cell_row_off, uint32_t n_cells, uint64_t n_reads)
{
    if (cell_row_off[0] != 0 || cell_row_off[n_cells] != n_reads)
        return fail(OEM_ERR_ARG, "%s: cell_row_off must span [0, n_reads]", who);
    for (uint32_t c = 0; c < n_cells; ++c)
        if (cell_row_off[c + 1] < cell_row_off[c])
            return fail(OEM_ERR_ARG, "%s: cell_row_off not non-decreasing at cell %u", who, c);
    return OEM_OK;
}

// ---- the cut and the workers
std::vector<std::pair<uint32_t, uint32_t>> cut_cells_groups(const uint64_t *cell_off, uint32_t n_cells, const uint64_t *ptr,
                                                            uint32_t n_txps)
{
    const auto at = [ptr](uint64_t i) { return ptr ? ptr[i] : i; }; // (no ptr: the entries are counted themselves)
    const uint64_t nnz = n_cells ? at(cell_off[n_cells]) - at(cell_off[0]) : 0;
    // Cells are independent problems, so a large experiment is cut into groups of consecutive cells
    // that bound the batched store (transcript space < 2^32, <= 2^30 alignments, and the layout
    // builder's tile x bucket table); each group is one batched run on the device.
    const uint64_t max_group_nnz = cells_max_group_nnz();
    std::vector<std::pair<uint32_t, uint32_t>> groups;
    uint32_t c0 = 0;
    while (c0 < n_cells) {
        uint32_t c1 = c0 + 1;
        while (c1 < n_cells) {
            const uint64_t cells = (uint64_t)(c1 + 1 - c0);
            const uint64_t reads = cell_off[c1 + 1] - cell_off[c0];
            const uint64_t gnnz = at(cell_off[c1 + 1]) - at(cell_off[c0]);
            if (!cells_group_fits(cells, reads, gnnz, n_txps, max_group_nnz)) break;
            ++c1;
        }
        groups.emplace_back(c0, c1);
        c0 = c1;
    }
    // One large group only (BASELINE configs[4]'s slice of one GPU: 625 cells, 250 M alignments, 2 GB of caller arrays):
    // a quarter of the cells is cut off as a group of its own, so that the second worker uploads and lays out the rest
    // under the head's EM loop instead of the device idling through the whole upload and layout build (~70 ms of a
    // 0.67 s call).  Measured (scripts/cells_groups_exp.sh, three rounds): heads of 40 / 80 / 160 / 312 of 625 cells
    // +7 / -0.5 / -3.4 / -0.5 % against one group -- a small head's own loop runs its few tiles badly, two halves just
    // share the device.
    if (groups.size() == 1 && n_cells >= (uint64_t)knob("OEM_CELLS_SPLIT_CELLS", 64) &&
        nnz >= (uint64_t)knob("OEM_CELLS_SPLIT_NNZ", 64l << 20)) { // testing build: split small calls too
        const long head = knob("OEM_CELLS_HEAD", (long)(kCellsHeadDiv ? n_cells / kCellsHeadDiv : 0));
        if (head >= 2 && (uint32_t)head + 2 <= n_cells) {
            groups.clear();
            groups.emplace_back(0u, (uint32_t)head);
            groups.emplace_back((uint32_t)head, n_cells);
        }
    }
    return groups;
}

int run_cells_workers(const char *who, CellsRun run, const std::vector<std::pair<uint32_t, uint32_t>> &groups,
                      const std::function<int(size_t, const CellsRun &, CellsGroupPath *)> &one)
{
    // Groups are independent runs.  With several of them two host threads draw groups from one counter, each group
    // on its own stream: one group's upload, layout build and read-back run under the other's EM loop, and the tail
    // of a loop -- the few cells that run into max_iter, a handful of live tiles per pass -- shares the device with
    // the other group's full passes instead of leaving it idle (single_cell.rs:96-150 runs its cells on N worker
    // threads for the same reason).
    std::vector<CellsGroupPath> paths(groups.size()); // (each group's slot is written by the worker that runs it)
    for (size_t g = 0; g < groups.size(); ++g) paths[g] = CellsGroupPath{groups[g].first, groups[g].second, 0, LaunchRecord()};
    CellsTiming timing;
    run.timing = &timing;
    std::atomic<size_t> next{0};
    constexpr int kMaxWorkers = 4;
    int n_workers = (int)knob("OEM_CELLS_WORKERS", 2);
    if (n_workers > kMaxWorkers) n_workers = kMaxWorkers;
    if ((size_t)n_workers > groups.size()) n_workers = (int)groups.size();
    if (n_workers < 1) n_workers = 1;
    int rcs[kMaxWorkers] = {OEM_OK, OEM_OK, OEM_OK, OEM_OK}; // each worker's own; read by the others only after the join
    std::atomic<bool> failed{false};                         // ... and this is what they stop on
    std::string errs[kMaxWorkers];
    size_t fail_group[kMaxWorkers] = {~(size_t)0, ~(size_t)0, ~(size_t)0, ~(size_t)0}; // (groups are drawn in order: the lowest
                                                                                      // failed group is the same every time)
    auto work = [&](int wk) {
        if (wk != 0 && hipSetDevice(run.device) != hipSuccess) {
            rcs[wk] = OEM_ERR_HIP;
            errs[wk] = "hipSetDevice failed in a per-cell worker";
            failed.store(true);
            return;
        }
        try {
            for (;;) {
                const size_t g = next.fetch_add(1);
                if (g >= groups.size() || failed.load()) break;
                rcs[wk] = one(g, run, &paths[g]);
                if (rcs[wk] != OEM_OK) fail_group[wk] = g;
                if (rcs[wk] != OEM_OK) break;
            }
        } catch (const std::exception &e) {
            rcs[wk] = fail(OEM_ERR_OOM, "per-cell worker: %s", e.what());
        } catch (...) {
            rcs[wk] = fail(OEM_ERR_STATE, "per-cell worker: unknown C++ exception");
        }
        if (rcs[wk] != OEM_OK) failed.store(true);
        if (rcs[wk] != OEM_OK && errs[wk].empty()) errs[wk] = last_error_text(); // (the message is thread-local)
    };
    {
        struct Joiner { // (a std::thread constructor that throws must not leave joinable threads behind)
            std::vector<std::thread> th;
            ~Joiner() { for (auto &t : th) if (t.joinable()) t.join(); }
        } pool;
        try {
            for (int wk = 1; wk < n_workers; ++wk) pool.th.emplace_back(work, wk);
        } catch (...) { // fewer threads: the ones that started take all the groups
        }
        work(0);
    }
    t_cells_loop_ms = timing.loop_ms();
    t_cells_batched_passes = timing.passes;
    t_cells_paths = std::move(paths);
    int first = -1;
    for (int wk = 0; wk < kMaxWorkers; ++wk)
        if (rcs[wk] != OEM_OK && (first < 0 || fail_group[wk] < fail_group[first])) first = wk;
    if (first >= 0) return fail(rcs[first], "%s", errs[first].c_str());
    return OEM_OK;
}

namespace {

// ---- the one-call form
// The caller's arrays of one call.
struct CellsInput {
    const uint64_t *cell_row_off;
    uint32_t n_cells;
    const uint64_t *row_ptr;
    const uint32_t *tid;
    const float *as_prob;
    const double *cov_prob;
    uint64_t n_reads, nnz;
};

// A group of a one-call run with what it owns: the rebased offsets and, with the coverage model, the CSR that stays on
// the device for the store.
struct CellsSlice {
    CellsGroup g;
    std::vector<uint64_t> off_v, rp_v, aoff_v;
    ResidentCsr res;
};

// Cells [c0, c1) of the call as a group (the sink is the caller's to fill in).
void slice_cells(const CellsInput &in, const CellsRun &run, uint32_t c0, uint32_t c1, CellsSlice *sl)
{
    CellsGroup &g = sl->g;
    const uint32_t n_cells = c1 - c0;
    const uint64_t r0 = in.cell_row_off[c0], r1 = in.cell_row_off[c1];
    const uint64_t a0 = in.row_ptr[r0], a1 = in.row_ptr[r1];
    const uint64_t n_reads = r1 - r0;
    // The group's own offsets.  A group that starts at read 0 (the whole experiment, when it fits one group)
    // takes the caller's arrays as they are: rebasing 31 M row offsets of a 625-cell batch into a fresh
    // 250 MB vector cost ~60 ms of page faults, 7 % of the call.  Later groups rebase on a few threads.
    g.cell_row_off = in.cell_row_off + c0;
    g.row_ptr = in.row_ptr;
    if (r0 != 0 || a0 != 0) {
        sl->off_v.resize((size_t)n_cells + 1);
        sl->rp_v.resize(n_reads + 1);
        for (uint32_t c = 0; c <= n_cells; ++c) sl->off_v[c] = in.cell_row_off[c0 + c] - r0;
        unsigned nt = std::thread::hardware_concurrency();
        if (nt > 16) nt = 16;
        if (nt < 1 || n_reads < (1u << 20)) nt = 1;
        auto rebase = [&](unsigned k) {
            const uint64_t b = (n_reads + 1) * k / nt, e = (n_reads + 1) * (k + 1) / nt;
            for (uint64_t r = b; r < e; ++r) sl->rp_v[r] = in.row_ptr[r0 + r] - a0;
        };
        if (nt == 1) {
            rebase(0);
        } else {
            std::vector<std::thread> th;
            for (unsigned k = 0; k < nt; ++k) th.emplace_back(rebase, k);
            for (auto &t : th) t.join();
        }
        g.cell_row_off = sl->off_v.data();
        g.row_ptr = sl->rp_v.data();
    }
    // the cells' first alignments within the group
    sl->aoff_v.resize((size_t)n_cells + 1);
    for (uint32_t c = 0; c <= n_cells; ++c) sl->aoff_v[c] = g.row_ptr[g.cell_row_off[c]];
    g.cell_aln_off = sl->aoff_v.data();
    g.n_cells = n_cells;
    g.n_reads = n_reads;
    g.nnz = a1 - a0;
    g.first_cell = c0;
    g.tid = in.tid ? in.tid + a0 : nullptr;
    g.as_prob = in.as_prob ? in.as_prob + a0 : nullptr;
    g.cov_prob = in.cov_prob ? in.cov_prob + a0 : nullptr;
    if (run.cov) {
        g.aln_start = run.cov->aln_start + a0;
        g.aln_end = run.cov->aln_end + a0;
        g.out_cov_prob = run.cov->out_cov_prob ? run.cov->out_cov_prob + a0 : nullptr;
        g.resident = &sl->res;
    }
}

// The body of both per-cell entry points (`who` names the caller in messages): argument checks, the NaN-coverage
// fix-up, the cut into groups and the workers; every group hands its results to `sink`.
// (`dense`: the caller's n_cells x n_txps matrix, or `blocks`: one SparseBlock per group, in group = cell order).
int run_cells(const char *who, CellsInput in, CellsRun run, double *dense, std::vector<SparseBlock> *blocks, oem_run_info *infos)
{
    const uint64_t *cell_row_off = in.cell_row_off, *row_ptr = in.row_ptr;
    const uint32_t n_cells = in.n_cells, n_txps = run.n_txps;
    const uint64_t n_reads = in.n_reads, nnz = in.nnz;
    if (!cell_row_off || !row_ptr || (n_cells && !dense && !blocks)) return fail(OEM_ERR_ARG, "%s: NULL argument", who);
    if (n_txps == 0) return fail(OEM_ERR_ARG, "%s: n_txps is 0", who);
    OEM_TRY(check_cell_row_off(who, cell_row_off, n_cells, n_reads));
    if (nnz > 0 && (!in.tid || !in.as_prob)) return fail(OEM_ERR_ARG, "%s: tid/as_prob is NULL", who);
    t_cells_loop_ms = 0.0;
    t_cells_batched_passes = 0;
    t_cells_paths.clear();
    StageTimer tm_all;
    OEM_TRY(validate_csr(row_ptr, in.tid, n_reads, nnz, n_txps)); // all cells at once, on several host threads
    tm_all.lap("cells: range checks");
    if (run.cov) { // the per-call part of the coverage model (the annotation), shared by the groups
        OEM_TRY(ensure_device(run.device));
        if (nnz) OEM_TRY(cells_coverage_setup(run.cov));
        tm_all.lap("cells: coverage set-up");
    }
    // a read with a NaN coverage probability is dropped (em.rs:115), on every path below: the batched
    // groups create their stores directly, not through oem_store_create
    std::vector<double> cov_fixed;
    if (in.cov_prob && zero_nan_rows(row_ptr, in.cov_prob, n_reads, nnz, &cov_fixed)) in.cov_prob = cov_fixed.data();

    const std::vector<std::pair<uint32_t, uint32_t>> groups = cut_cells_groups(cell_row_off, n_cells, row_ptr, n_txps);
    if (blocks) blocks->assign(groups.size(), SparseBlock());
    OEM_TRY(run_cells_workers(who, run, groups, [&](size_t g, const CellsRun &grun, CellsGroupPath *path) -> int {
        bool batched = false;
        CellsSlice sl;
        slice_cells(in, grun, groups[g].first, groups[g].second, &sl);
        sl.g.out_dense = dense ? dense + (uint64_t)groups[g].first * n_txps : nullptr;
        sl.g.blk = blocks ? &(*blocks)[g] : nullptr;
        sl.g.infos = infos ? infos + groups[g].first : nullptr;
        sl.g.launch = &path->launch;
        const int rc = run_cells_group(grun, sl.g, &batched);
        path->batched = batched ? 1u : 0u;
        return rc;
    }));
    tm_all.lap("cells: all groups");
    return OEM_OK;
}

// The body of both sparse entry points: the groups' blocks become one oem_cells_result.
int run_cells_sparse(const char *who, const CellsInput &in, const CellsRun &run, oem_cells_result **out)
{
    std::unique_ptr<oem_cells_result> r(new oem_cells_result());
    r->n_cells = in.n_cells;
    r->infos.resize(in.n_cells);
    std::vector<SparseBlock> blocks;
    OEM_TRY(run_cells(who, in, run, nullptr, &blocks, r->infos.data()));
    OEM_TRY(cells_result_from_blocks(who, blocks, r.get()));
    *out = r.release();
    return OEM_OK;
}

} // namespace

int cells_result_from_blocks(const char *who, std::vector<SparseBlock> &blocks, oem_cells_result *r)
{
    const uint32_t n_cells = r->n_cells;
    r->cell_off.assign((size_t)n_cells + 1, 0);
    uint32_t c = 0;
    for (const SparseBlock &b : blocks) {
        uint64_t n = 0;
        for (uint32_t k : b.counts) {
            if (c >= n_cells) break;
            r->cell_off[c + 1] = r->cell_off[c] + k;
            n += k;
            ++c;
        }
        if (n != b.col.size() || n != b.val.size())
            return fail(OEM_ERR_STATE, "%s: a group's entries do not match its counts", who);
    }
    if (c != n_cells) return fail(OEM_ERR_STATE, "%s: the groups' results cover %u of %u cells", who, c, n_cells);
    r->n_entries = r->cell_off[n_cells];
    r->blocks = std::move(blocks);
    return OEM_OK;
}

} // namespace oem

using namespace oem;

// ---- entry points
extern "C" int oem_em_run_cells(const uint64_t *cell_row_off, uint32_t n_cells, const uint64_t *row_ptr,
                                const uint32_t *tid, const float *as_prob, const double *cov_prob,
                                uint64_t n_reads, uint64_t nnz, uint32_t n_txps, int device,
                                uint32_t max_iter, double conv_thresh, double *out,
                                oem_run_info *infos)
{
    OEM_API_BEGIN
    return run_cells("oem_em_run_cells", CellsInput{cell_row_off, n_cells, row_ptr, tid, as_prob, cov_prob, n_reads, nnz},
                     CellsRun{n_txps, device, max_iter, conv_thresh}, out, nullptr, infos);
    OEM_API_END("oem_em_run_cells")
}

extern "C" int oem_em_run_cells_sparse(const uint64_t *cell_row_off, uint32_t n_cells, const uint64_t *row_ptr,
                                       const uint32_t *tid, const float *as_prob, const double *cov_prob,
                                       uint64_t n_reads, uint64_t nnz, uint32_t n_txps, int device,
                                       uint32_t max_iter, double conv_thresh, oem_cells_result **out)
{
    OEM_API_BEGIN
    if (!out) return fail(OEM_ERR_ARG, "oem_em_run_cells_sparse: out is NULL");
    *out = nullptr;
    return run_cells_sparse("oem_em_run_cells_sparse", CellsInput{cell_row_off, n_cells, row_ptr, tid, as_prob, cov_prob, n_reads, nnz},
                            CellsRun{n_txps, device, max_iter, conv_thresh}, out);
    OEM_API_END("oem_em_run_cells_sparse")
}

// single_cell.rs:117-160 from the built store on: every cell's coverage model and its EM in one call.  Per group of
// cells the caller's arrays go up once; the coverage column is computed and turned into the f64 weights on the device
// and the group's store takes the buffers over, so neither the column nor the weights cross PCIe.
extern "C" int oem_em_run_cells_coverage_sparse(const uint64_t *cell_row_off, uint32_t n_cells, const uint64_t *row_ptr,
                                                const uint32_t *tid, const float *as_prob, const uint32_t *aln_start,
                                                const uint32_t *aln_end, const uint64_t *txp_len, uint64_t n_reads,
                                                uint64_t nnz, uint32_t n_txps, uint32_t bin_width, int model,
                                                double growth_rate, int device, uint32_t max_iter, double conv_thresh,
                                                double *out_cov_prob, oem_cells_result **out)
{
    OEM_API_BEGIN
    const char *who = "oem_em_run_cells_coverage_sparse";
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (!cell_row_off || !row_ptr || !txp_len || (nnz && (!tid || !as_prob || !aln_start || !aln_end)))
        return fail(OEM_ERR_ARG, "%s: NULL argument", who);
    OEM_TRY(check_cells_coverage_args(who, bin_width, model, n_txps, nnz, n_reads));
    // (run_cells checks cell_row_off and the CSR before any device work)
    CellsCoverage cc;
    cc.aln_start = aln_start;
    cc.aln_end = aln_end;
    cc.txp_len = txp_len;
    cc.n_txps = n_txps;
    cc.bin_width = bin_width;
    cc.model = model;
    cc.growth_rate = growth_rate;
    cc.out_cov_prob = out_cov_prob;
    return run_cells_sparse(who, CellsInput{cell_row_off, n_cells, row_ptr, tid, as_prob, nullptr, n_reads, nnz},
                            CellsRun{n_txps, device, max_iter, conv_thresh, &cc}, out);
    OEM_API_END("oem_em_run_cells_coverage_sparse")
}

extern "C" int oem_cells_result_dims(const oem_cells_result *r, uint32_t *n_cells, uint64_t *n_entries)
{
    if (!r) return fail(OEM_ERR_ARG, "oem_cells_result_dims: NULL result");
    if (n_cells) *n_cells = r->n_cells;
    if (n_entries) *n_entries = r->n_entries;
    return OEM_OK;
}

extern "C" int oem_cells_result_copy(const oem_cells_result *r, uint64_t *cell_off, uint32_t *col, float *val,
                                     oem_run_info *infos)
{
    if (!r) return fail(OEM_ERR_ARG, "oem_cells_result_copy: NULL result");
    if (cell_off) std::memcpy(cell_off, r->cell_off.data(), sizeof(uint64_t) * r->cell_off.size());
    uint64_t at = 0;
    for (const SparseBlock &b : r->blocks) {
        if (b.col.empty()) continue;
        if (col) std::memcpy(col + at, b.col.data(), sizeof(uint32_t) * b.col.size());
        if (val) std::memcpy(val + at, b.val.data(), sizeof(float) * b.val.size());
        at += b.col.size();
    }
    if (infos && !r->infos.empty()) std::memcpy(infos, r->infos.data(), sizeof(oem_run_info) * r->infos.size());
    return OEM_OK;
}

extern "C" void oem_cells_result_destroy(oem_cells_result *r)
{
    delete r;
}
