// oem_cells_stream.hip -- the per-cell session (oem_cells_stream_*): cells are pushed one by one, from any number of
// threads (single_cell.rs:96-193: N workers each pop one cell and build its store), staged in host memory, cut into
// groups and run through the per-cell driver's unit of work (a CellsGroup, run_cells_group, oem_cells.hip) by two
// device workers while later cells still arrive.
//
//   push      checks the cell on the calling thread, reserves its place in the open group under the session lock
//             (ticket, read and alignment offsets) and copies the arrays outside the lock.  The open group is closed --
//             handed to the workers -- once it holds group_nnz alignments or group_cells cells, when the next cell would
//             break the driver's group rule (cells_group_fits), or when a push has to wait for room.
//   staging   one allocation per group: the cells' row pointers AS PUSHED (each cell's n + 1 entries, starting at 0),
//             ids, probabilities and, for the coverage model, coordinates.  Pinned (page-locked) memory, so that the
//             upload of one group is an asynchronous copy under the other worker's EM loop; pageable when the pinned
//             allocation fails.  Arenas are reused from group to group.
//   worker    uploads the row pointers with the per-cell read / alignment offset tables; k_stream_row_ptr builds the
//             group's u32 row pointers and its cell_row_off on the device and range-checks them in the same pass (no
//             host pass over the reads of the group).  The store adopts these buffers (ResidentCsr), and
//             run_cells_group does the rest exactly as for a group of a one-call run, fallbacks included.
//   finish    closes the last group, joins the workers and concatenates the groups' blocks in ticket order.
//
// A RECORDS session (oem_cells_stream_set_filters, oem_cells_stream_push_records) stages the cells' alignment records
// instead, 40 B each, with each cell's group offsets where the row pointers would be; the budgets count records.  Its
// worker concatenates the group offsets on the host (8 B per read) and runs the records-to-group step of
// oem_em_run_cells_records_sparse (run_records_group, oem_cells_records.hip) straight from the page-locked staging:
// filter, per-cell offsets and discard tables on the device, then run_cells_group.  k_stream_row_ptr is not needed there.
//
// A BARCODED session (oem_cells_stream_set_barcodes, oem_cells_stream_push_barcodes) takes batches of records cut at any
// position and finds the cells itself (oem_cells_barcodes_stream.hip).  Nothing of it is staged here: its groups come
// from its device arena as closures (Group::dev_run) that the same two workers run, in the same result slots.  Its
// ANY-ORDER form (oem_cells_stream_set_barcodes_any_order, oem_cells_barcodes_sort_stream.hip) is the same session under
// another rule: a barcode that comes back is the same cell, so its groups come only at finish.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "oem_cells.h"
#include "oem_cells_barcodes_stream.h"

namespace oem {
namespace {

// Defaults of oem_cells_stream_opts.  group_nnz is the best point of the one sweep that exists (scripts/
// cells_stream_bench.py, profiles/cells_stream_bench.json: 625 cells x 400 k alignments from 8 pushing threads, 8 / 16 /
// 32 / 64 / 128 Mi alignments per group: 1.15 / 0.83 / 0.83 / 0.90 / 0.99 s) -- larger groups start the device late,
// smaller ones run their few tiles badly, as the head-split experiment of run_cells had it.  group_cells and
// max_staged_nnz (two groups' worth) have NOT been measured.
constexpr uint64_t kDefaultGroupNnz = 32ull << 20;
constexpr uint32_t kDefaultGroupCells = 65535; // (the driver's own bound: gridDim.y of the per-cell kernels)
constexpr int kStreamWorkers = 2;              // as run_cells: one group's upload and layout under the other's loop
constexpr int kPinnedArenas = 4;               // open + queued + one per worker; further arenas are pageable
constexpr uint64_t kFirstArenaNnz = 1ull << 20; // an arena starts small and grows x4 up to the group's size

// One lane per read of the group: its cell by binary search in the read-offset table, then the group-wide u32 row
// pointer from the cell's own (0-based) one, range-checked on the way.  The first n_cells + 1 lanes also write the
// group's cell_row_off.  rp_local holds every cell's n + 1 entries one after the other: cell c starts at
// read_off[c] + c.
__global__ __launch_bounds__(256) void k_stream_row_ptr(const unsigned long long *__restrict__ rp_local,
                                                        const unsigned long long *__restrict__ read_off,
                                                        const unsigned long long *__restrict__ aln_off, uint32_t n_cells,
                                                        uint64_t n_reads, uint32_t *__restrict__ row_ptr,
                                                        unsigned long long *__restrict__ cell_row_off, uint32_t *__restrict__ err)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= n_cells) cell_row_off[r] = read_off[r];
    if (r == 0) row_ptr[n_reads] = (uint32_t)aln_off[n_cells];
    if (r >= n_reads) return;
    uint32_t a = 0, b = n_cells; // last cell whose first read is <= r (empty cells share offsets: never the last)
    while (b - a > 1) {
        const uint32_t m = (a + b) >> 1;
        if (read_off[m] <= r) a = m;
        else b = m;
    }
    const uint64_t first = read_off[a], i = r - first;
    const uint64_t cell_reads = read_off[a + 1] - first, cell_nnz = aln_off[a + 1] - aln_off[a];
    const unsigned long long *loc = rp_local + first + a;
    const uint64_t v0 = loc[i], v1 = loc[i + 1];
    const bool bad = v1 < v0 || v1 > cell_nnz || (i == 0 && v0 != 0) || (i + 1 == cell_reads && v1 != cell_nnz);
    if (bad) atomicOr(err, 1u);
    row_ptr[r] = (uint32_t)(aln_off[a] + (bad ? 0 : v0));
}

// The host staging of one group, one allocation.
struct Staging {
    void *base = nullptr;
    bool pinned = false;
    uint64_t cap_nnz = 0, cap_rp = 0;
    uint64_t *rp = nullptr;
    uint32_t *tid = nullptr, *start = nullptr, *end = nullptr;
    float *p = nullptr;
    oem_aln_record *rec = nullptr; // a records session: the records (cap_nnz of them); rp holds the group offsets
    Staging() = default;
    Staging(const Staging &) = delete;
    Staging &operator=(const Staging &) = delete;
    ~Staging()
    {
        if (pinned) (void)hipHostFree(base);
        else free(base);
    }
    static std::unique_ptr<Staging> make(uint64_t cap_nnz, uint64_t cap_rp, bool coverage, bool try_pinned, bool records)
    {
        std::unique_ptr<Staging> s(new Staging());
        const size_t bytes = sizeof(uint64_t) * cap_rp + (records ? sizeof(oem_aln_record) : coverage ? 16 : 8) * cap_nnz + 64;
        if (try_pinned && hipHostMalloc(&s->base, bytes, hipHostMallocPortable) == hipSuccess) {
            s->pinned = true;
        } else {
            if (try_pinned) (void)hipGetLastError();
            s->base = malloc(bytes);
            if (!s->base) throw std::bad_alloc();
        }
        s->cap_nnz = cap_nnz;
        s->cap_rp = cap_rp;
        char *q = (char *)s->base;
        s->rp = (uint64_t *)q;
        q += sizeof(uint64_t) * cap_rp;
        if (records) {
            s->rec = (oem_aln_record *)q;
            return s;
        }
        s->tid = (uint32_t *)q;
        q += sizeof(uint32_t) * cap_nnz;
        s->p = (float *)q;
        q += sizeof(float) * cap_nnz;
        if (coverage) {
            s->start = (uint32_t *)q;
            q += sizeof(uint32_t) * cap_nnz;
            s->end = (uint32_t *)q;
        }
        return s;
    }
};

struct Group {
    std::unique_ptr<Staging> st;
    size_t index = 0;          // the group's number: its place in the result
    uint64_t first_ticket = 0;
    uint32_t n_cells = 0;
    uint64_t n_reads = 0, nnz = 0;
    std::vector<uint64_t> read_off{0}, aln_off{0}; // n_cells + 1 each
    int pending = 0;           // pushes still copying into the staging
    std::vector<uint64_t> host_rp; // the concatenated row pointers, only when the host layout builder asks
    StreamGroupRun dev_run;        // a barcoded session's group: nothing is staged, it runs from the session's device arena
    uint64_t rp_used() const { return n_reads + n_cells; }

    static const uint64_t *host_row_ptr(void *ctx)
    {
        Group *g = (Group *)ctx;
        try {
            if (g->host_rp.empty()) {
                g->host_rp.resize(g->n_reads + 1);
                for (uint32_t c = 0; c < g->n_cells; ++c) {
                    const uint64_t r0 = g->read_off[c], n = g->read_off[c + 1] - r0;
                    const uint64_t *loc = g->st->rp + r0 + c;
                    for (uint64_t i = 0; i < n; ++i) g->host_rp[r0 + i] = g->aln_off[c] + loc[i];
                }
                g->host_rp[g->n_reads] = g->nnz;
            }
            return g->host_rp.data();
        } catch (...) {
            return nullptr;
        }
    }
};

using GroupResult = StreamGroupResult; // (tables: a records session's discard tables)

// what a push stages: a cell's CSR, or its records
struct CellArrays {
    const uint64_t *rp = nullptr; // row pointers, or the group offsets of the records
    const uint32_t *tid = nullptr;
    const float *p = nullptr;
    const uint32_t *start = nullptr, *end = nullptr;
    const oem_aln_record *rec = nullptr;
};

} // namespace
} // namespace oem

using namespace oem;

struct oem_cells_stream {
    oem_cells_stream_opts o;
    uint64_t group_nnz = 0, max_staged = 0;
    uint32_t group_cells = 0;
    std::vector<uint64_t> txp_len;
    CellsCoverage cov;
    bool records_mode = false; // set by oem_cells_stream_set_filters before the first push
    RecordsFilter rf;
    BarcodesStream *bc = nullptr; // set by oem_cells_stream_set_barcodes: the barcoded form of a records session

    mutable std::mutex mu;
    std::condition_variable cv_work, cv_space, cv_copy;
    std::unique_ptr<Group> open;
    std::deque<std::unique_ptr<Group>> queue;
    std::vector<std::unique_ptr<Staging>> pool;
    std::vector<GroupResult> results; // by group index
    int arenas_pinned = 0;
    uint64_t arena_nnz = 0, arena_rp = 0; // what a new group's arena starts with (the high-water mark so far)
    uint64_t next_ticket = 0, total_nnz = 0, staged_nnz = 0;
    uint64_t groups_started = 0, groups_before_finish = 0, groups_batched = 0, blocked_us = 0;
    int pushes_in_flight = 0;
    bool finish_called = false, stop = false, cancel = false;
    int sticky_rc = OEM_OK;
    std::string sticky_msg;
    std::vector<std::thread> workers;

    uint64_t full_arena_nnz() const { return group_nnz + group_nnz / 8 + 4096; }
    uint64_t full_arena_rp() const { return full_arena_nnz() / 2 + 65536 + 8; }

    // (mu held) an arena of at least this capacity: from the pool, or a new one
    std::unique_ptr<Staging> take_arena(uint64_t need_nnz, uint64_t need_rp)
    {
        for (size_t k = 0; k < pool.size(); ++k)
            if (pool[k]->cap_nnz >= need_nnz && pool[k]->cap_rp >= need_rp) {
                std::unique_ptr<Staging> s = std::move(pool[k]);
                pool.erase(pool.begin() + k);
                return s;
            }
        if (!pool.empty()) { // too small for this group: not kept
            if (pool.back()->pinned) --arenas_pinned;
            pool.pop_back();
        }
        const bool try_pinned = arenas_pinned < kPinnedArenas && hipSetDevice(o.device) == hipSuccess;
        StageTimer tm;
        std::unique_ptr<Staging> s = Staging::make(need_nnz, need_rp, o.coverage != 0, try_pinned, records_mode);
        if (s->pinned) ++arenas_pinned;
        if (tm.on)
            fprintf(stderr, "[oem] stream: new %s arena for %llu alignments, %llu row pointers\n", s->pinned ? "pinned" : "pageable",
                    (unsigned long long)need_nnz, (unsigned long long)need_rp);
        tm.lap("stream: arena allocation");
        return s;
    }
    void give_arena(std::unique_ptr<Staging> s)
    {
        if (!s) return;
        if (pool.size() < (size_t)kPinnedArenas) {
            pool.push_back(std::move(s));
        } else if (s->pinned) {
            --arenas_pinned;
        }
    }
    // (mu held) the open group goes to the workers
    void close_open()
    {
        if (!open) return;
        if (open->n_cells == 0) {
            give_arena(std::move(open->st));
            open.reset();
            return;
        }
        queue.push_back(std::move(open));
        cv_work.notify_one();
    }
    void set_sticky(int rc, const char *msg)
    {
        if (sticky_rc != OEM_OK) return;
        sticky_rc = rc;
        sticky_msg = msg;
    }

    int run_group(Group &g, hipStream_t st, GroupResult *out, bool *batched, bool *uploaded);
    int run_records(Group &g, GroupResult *out, bool *batched);
    int push_cell(const char *who, bool records, const CellArrays &a, uint64_t n_reads, uint64_t nnz, uint64_t *out_ticket);
    void work(int wk);
};

// One closed group on a worker's stream: upload, row pointers on the device, then the driver's unit of work.
int oem_cells_stream::run_group(Group &g, hipStream_t st, GroupResult *out, bool *batched, bool *uploaded)
{
    StageTimer tm;
    const Staging &sg = *g.st;
    const uint32_t nc = g.n_cells;
    ResidentCsr res;
    DevBuf<unsigned long long> d_rp, d_tab; // the cells' row pointers as pushed; read_off | aln_off | cell_row_off
    DevBuf<uint32_t> d_err;
    uint32_t h_err = 0;
    OEM_TRY(dev_alloc(&res.row_ptr, g.n_reads + 1, nullptr));
    OEM_TRY(dev_alloc(&d_rp.p, g.rp_used(), nullptr));
    OEM_TRY(dev_alloc(&d_tab.p, 3 * ((size_t)nc + 1), nullptr));
    OEM_TRY(dev_alloc(&d_err.p, 1, nullptr));
    OEM_HIP(hipMemcpyAsync(d_rp.p, sg.rp, sizeof(uint64_t) * g.rp_used(), hipMemcpyHostToDevice, st));
    OEM_HIP(hipMemcpyAsync(d_tab.p, g.read_off.data(), sizeof(uint64_t) * (nc + 1), hipMemcpyHostToDevice, st));
    OEM_HIP(hipMemcpyAsync(d_tab.p + nc + 1, g.aln_off.data(), sizeof(uint64_t) * (nc + 1), hipMemcpyHostToDevice, st));
    OEM_HIP(hipMemsetAsync(d_err.p, 0, sizeof(uint32_t), st));
    const uint64_t lanes = std::max<uint64_t>(g.n_reads, (uint64_t)nc + 1);
    hipLaunchKernelGGL(k_stream_row_ptr, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, d_rp.p, d_tab.p,
                       d_tab.p + nc + 1, nc, g.n_reads, res.row_ptr, d_tab.p + 2 * ((size_t)nc + 1), d_err.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpyAsync(&h_err, d_err.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (!o.coverage) { // (with the coverage model the group's coverage step uploads ids and coordinates and writes w64)
        OEM_TRY(dev_alloc(&res.tid, g.nnz, nullptr));
        OEM_TRY(dev_alloc(&res.w32, g.nnz, nullptr));
        if (g.nnz) {
            OEM_HIP(hipMemcpyAsync(res.tid, sg.tid, sizeof(uint32_t) * g.nnz, hipMemcpyHostToDevice, st));
            OEM_HIP(hipMemcpyAsync(res.w32, sg.p, sizeof(float) * g.nnz, hipMemcpyHostToDevice, st));
        }
    }
    OEM_HIP(hipStreamSynchronize(st));
    if (h_err)
        return fail(OEM_ERR_STATE, "oem_cells_stream: the staged row pointers of the group of cell %llu fail the device's range check",
                    (unsigned long long)g.first_ticket);
    d_rp.reset();
    tm.lap("stream: upload + row pointers");
    {
        std::lock_guard<std::mutex> lk(mu);
        staged_nnz -= g.nnz;
        *uploaded = true;
    }
    cv_space.notify_all();

    res.host_row_ptr = &Group::host_row_ptr;
    res.host_row_ptr_ctx = &g;
    out->infos.assign(nc, oem_run_info{});
    CellsGroup cg; // no host row_ptr (the host layout builder asks `res` for one), cell_row_off on the device too
    cg.n_cells = nc;
    cg.n_reads = g.n_reads;
    cg.nnz = g.nnz;
    cg.first_cell = g.first_ticket;
    cg.cell_row_off = g.read_off.data();
    cg.cell_aln_off = g.aln_off.data();
    cg.tid = sg.tid;
    cg.as_prob = sg.p;
    cg.aln_start = sg.start;
    cg.aln_end = sg.end;
    cg.resident = &res;
    cg.d_cell_row_off = d_tab.p + 2 * ((size_t)nc + 1);
    cg.blk = &out->blk;
    cg.infos = out->infos.data();
    CellsRun run{o.n_txps, o.device, o.max_iter, o.conv_thresh, o.coverage ? &cov : nullptr};
    OEM_TRY(run_cells_group(run, cg, batched));
    tm.lap("stream: group run");
    return OEM_OK;
}

// One closed group of a records session: the group-wide offsets, then the records-to-group step of the one-call form.
int oem_cells_stream::run_records(Group &g, GroupResult *out, bool *batched)
{
    const uint32_t nc = g.n_cells;
    std::vector<uint64_t> goff(g.n_reads + 1); // (reads = record groups, alignments = records)
    for (uint32_t c = 0; c < nc; ++c) {
        const uint64_t r0 = g.read_off[c], n = g.read_off[c + 1] - r0;
        const uint64_t *loc = g.st->rp + r0 + c;
        for (uint64_t i = 0; i < n; ++i) goff[r0 + i] = g.aln_off[c] + loc[i];
    }
    goff[g.n_reads] = g.nnz;
    out->infos.assign(nc, oem_run_info{});
    out->tables.assign(nc, oem_discard_table{});
    RecordsGroup rg;
    rg.records = g.st->rec;
    rg.pinned = g.st->pinned;
    rg.group_off = goff.data();
    rg.n_groups = g.n_reads;
    rg.cell_group_off = g.read_off.data();
    rg.n_cells = nc;
    rg.first_cell = g.first_ticket;
    rg.out_tables = out->tables.data();
    rg.blk = &out->blk;
    rg.infos = out->infos.data();
    CellsRun run{o.n_txps, o.device, o.max_iter, o.conv_thresh, o.coverage ? &cov : nullptr};
    return run_records_group("oem_cells_stream", run, rf, rg, batched);
}

void oem_cells_stream::work(int wk)
{
    hipStream_t st = nullptr;
    if (hipSetDevice(o.device) != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
        std::lock_guard<std::mutex> lk(mu);
        set_sticky(OEM_ERR_HIP, "oem_cells_stream: a device worker could not open its stream");
        st = nullptr;
    }
    for (;;) {
        std::unique_ptr<Group> g;
        bool skip;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv_work.wait(lk, [&] { return !queue.empty() || stop; });
            if (queue.empty()) break;
            g = std::move(queue.front());
            queue.pop_front();
            skip = cancel || sticky_rc != OEM_OK || !st;
            if (!skip) {
                ++groups_started;
                if (!finish_called) ++groups_before_finish;
            }
            cv_copy.wait(lk, [&] { return g->pending == 0; });
        }
        GroupResult res;
        bool batched = false, uploaded = false;
        int rc = OEM_OK;
        std::string msg;
        if (!skip) {
            try {
                rc = g->dev_run      ? g->dev_run(&res, &batched)
                     : records_mode ? run_records(*g, &res, &batched)
                                    : run_group(*g, st, &res, &batched, &uploaded);
            } catch (const std::bad_alloc &) {
                rc = fail(OEM_ERR_OOM, "oem_cells_stream: host allocation failed in a device worker");
            } catch (const std::exception &e) {
                rc = fail(OEM_ERR_STATE, "oem_cells_stream: %s", e.what());
            }
            if (rc != OEM_OK) msg = last_error_text(); // (the message is thread-local)
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!uploaded) staged_nnz -= g->nnz;
            if (rc != OEM_OK) set_sticky(rc, msg.c_str());
            else if (!skip) {
                results[g->index] = std::move(res);
                if (batched) ++groups_batched;
            }
            give_arena(std::move(g->st));
        }
        cv_space.notify_all();
    }
    if (st) {
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
    }
    (void)wk;
}

extern "C" int oem_cells_stream_create(const oem_cells_stream_opts *opts, const uint64_t *txp_len, oem_cells_stream **out)
{
    OEM_API_BEGIN
    const char *who = "oem_cells_stream_create";
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (!opts) return fail(OEM_ERR_ARG, "%s: opts is NULL", who);
    if (opts->n_txps == 0) return fail(OEM_ERR_ARG, "%s: n_txps is 0", who);
    if (opts->coverage > 1) return fail(OEM_ERR_ARG, "%s: coverage must be 0 or 1", who);
    for (uint32_t r : opts->reserved)
        if (r) return fail(OEM_ERR_ARG, "%s: a reserved word is not 0", who);
    if (opts->coverage) {
        if (!txp_len) return fail(OEM_ERR_ARG, "%s: coverage = 1 needs txp_len", who);
        OEM_TRY(check_cells_coverage_args(who, opts->bin_width, opts->model, opts->n_txps, 0, 0));
    }
    OEM_TRY(ensure_device(opts->device));
    std::unique_ptr<oem_cells_stream> s(new oem_cells_stream());
    s->o = *opts;
    s->group_nnz = opts->group_nnz ? opts->group_nnz : kDefaultGroupNnz;
    s->group_nnz = std::min(s->group_nnz, cells_max_group_nnz());
    s->group_cells = opts->group_cells ? std::min(opts->group_cells, kDefaultGroupCells) : kDefaultGroupCells;
    s->max_staged = opts->max_staged_nnz ? opts->max_staged_nnz : 2 * s->group_nnz; // not measured either
    s->arena_nnz = std::min(kFirstArenaNnz, s->full_arena_nnz());
    s->arena_rp = std::min(kFirstArenaNnz / 2 + 4096, s->full_arena_rp());
    if (opts->coverage) { // the per-session part of the coverage model (the annotation), shared by the groups
        s->txp_len.assign(txp_len, txp_len + opts->n_txps);
        s->cov.txp_len = s->txp_len.data();
        s->cov.n_txps = opts->n_txps;
        s->cov.bin_width = opts->bin_width;
        s->cov.model = opts->model;
        s->cov.growth_rate = opts->growth_rate;
        OEM_TRY(cells_coverage_setup(&s->cov));
    }
    oem_cells_stream *raw = s.get();
    try {
        for (int wk = 0; wk < kStreamWorkers; ++wk) raw->workers.emplace_back([raw, wk] { raw->work(wk); });
    } catch (...) {
        if (raw->workers.empty()) {
            return fail(OEM_ERR_STATE, "%s: no device worker could be started", who);
        } // (fewer threads: the ones that started take all the groups)
    }
    *out = s.release();
    return OEM_OK;
    OEM_API_END("oem_cells_stream_create")
}

// The session's half of a push (the cell has been checked by its entry point): the cell's place in the open group
// under the lock -- group rule, back-pressure, arena growth -- and the copy of its arrays outside it.  n_reads / nnz:
// reads and alignments, or record groups and records.
int oem_cells_stream::push_cell(const char *who, bool records, const CellArrays &a, uint64_t n_reads, uint64_t nnz,
                                uint64_t *out_ticket)
{
    std::unique_lock<std::mutex> lk(mu);
    ++pushes_in_flight;
    struct InFlight { // (mu is held whenever this scope is left)
        oem_cells_stream *s;
        ~InFlight() { --s->pushes_in_flight; }
    } in_flight{this};
    const uint64_t hard_nnz = cells_max_group_nnz();
    Group *g = nullptr;
    try {
        for (;;) {
            if (finish_called || cancel) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
            if (bc) return fail(OEM_ERR_STATE, "%s: a barcoded session takes batches through oem_cells_stream_push_barcodes", who);
            if (records != records_mode)
                return fail(OEM_ERR_STATE, records ? "%s: not a records session (oem_cells_stream_set_filters)"
                                                   : "%s: a records session takes cells through oem_cells_stream_push_records", who);
            if (sticky_rc != OEM_OK) return fail(sticky_rc, "%s", sticky_msg.c_str());
            if (next_ticket >= 0xffffffffull) return fail(OEM_ERR_STATE, "%s: a session holds fewer than 2^32 cells", who);
            g = open.get();
            // the driver's own group rule: the cell starts a new group when it would break the open one's
            if (g && g->n_cells > 0 && !cells_group_fits((uint64_t)g->n_cells + 1, g->n_reads + n_reads, g->nnz + nnz, o.n_txps, hard_nnz)) {
                close_open();
                continue;
            }
            // back-pressure; what waits in the open group goes to the workers first, or nothing would ever drain
            if (staged_nnz > 0 && staged_nnz + nnz > max_staged) {
                close_open();
                const auto t0 = std::chrono::steady_clock::now();
                cv_space.wait(lk);
                blocked_us += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
                continue;
            }
            if (!g) {
                std::unique_ptr<Group> ng(new Group());
                ng->st = take_arena(std::max(arena_nnz, nnz), std::max(arena_rp, n_reads + 1));
                ng->index = results.size();
                ng->first_ticket = next_ticket;
                results.emplace_back();
                open = std::move(ng);
                g = open.get();
            }
            if (g->nnz + nnz > g->st->cap_nnz || g->rp_used() + n_reads + 1 > g->st->cap_rp) {
                const bool full_size = g->st->cap_nnz >= full_arena_nnz() && g->st->cap_rp >= full_arena_rp();
                if (full_size && g->n_cells > 0) { // a full-sized arena is full: the group is large enough
                    close_open();
                    continue;
                }
                if (g->pending) { // pushes still copy into the arena: it cannot move yet
                    cv_copy.wait(lk);
                    continue;
                }
                // grow x4 towards the full size (or to what a single large cell needs); the staged part moves over
                uint64_t cn = g->st->cap_nnz, cr = g->st->cap_rp;
                while (cn < g->nnz + nnz) cn = std::max(cn * 4, g->nnz + nnz);
                while (cr < g->rp_used() + n_reads + 1) cr = std::max(cr * 4, g->rp_used() + n_reads + 1);
                if (g->nnz + nnz <= full_arena_nnz()) cn = std::min(cn, full_arena_nnz());
                if (g->rp_used() + n_reads + 1 <= full_arena_rp()) cr = std::min(cr, full_arena_rp());
                std::unique_ptr<Staging> old = std::move(g->st);
                g->st = take_arena(cn, cr);
                std::memcpy(g->st->rp, old->rp, sizeof(uint64_t) * g->rp_used());
                if (records) {
                    std::memcpy(g->st->rec, old->rec, sizeof(oem_aln_record) * g->nnz);
                } else {
                    std::memcpy(g->st->tid, old->tid, sizeof(uint32_t) * g->nnz);
                    std::memcpy(g->st->p, old->p, sizeof(float) * g->nnz);
                }
                if (!records && o.coverage) {
                    std::memcpy(g->st->start, old->start, sizeof(uint32_t) * g->nnz);
                    std::memcpy(g->st->end, old->end, sizeof(uint32_t) * g->nnz);
                }
                if (old->pinned) --arenas_pinned; // (released here: smaller than what groups need by now)
                old.reset();
                arena_nnz = std::min(std::max(arena_nnz, cn), full_arena_nnz());
                arena_rp = std::min(std::max(arena_rp, cr), full_arena_rp());
                continue;
            }
            g->read_off.reserve(g->read_off.size() + 1); // (so that taking the cell's place below cannot throw)
            g->aln_off.reserve(g->aln_off.size() + 1);
            break;
        }
    } catch (const std::bad_alloc &) { // staging could not be allocated: the session cannot keep its promise
        set_sticky(OEM_ERR_OOM, "oem_cells_stream_push: host allocation of the staging memory failed");
        cv_space.notify_all();
        return fail(OEM_ERR_OOM, "%s", sticky_msg.c_str());
    }
    // the cell's place: ticket, offsets; the arrays are copied outside the lock
    const uint64_t ticket = next_ticket++;
    const uint64_t rp_at = g->rp_used(), a_at = g->nnz;
    Staging *st = g->st.get();
    g->n_cells += 1;
    g->n_reads += n_reads;
    g->nnz += nnz;
    g->read_off.push_back(g->n_reads);
    g->aln_off.push_back(g->nnz);
    g->pending += 1;
    total_nnz += nnz;
    staged_nnz += nnz;
    if (g->nnz >= group_nnz || g->n_cells >= group_cells) close_open(); // (the worker waits for the copy below)
    lk.unlock();
    std::memcpy(st->rp + rp_at, a.rp, sizeof(uint64_t) * (n_reads + 1));
    if (nnz && records) {
        std::memcpy(st->rec + a_at, a.rec, sizeof(oem_aln_record) * nnz);
    } else if (nnz) {
        std::memcpy(st->tid + a_at, a.tid, sizeof(uint32_t) * nnz);
        std::memcpy(st->p + a_at, a.p, sizeof(float) * nnz);
        if (o.coverage) {
            std::memcpy(st->start + a_at, a.start, sizeof(uint32_t) * nnz);
            std::memcpy(st->end + a_at, a.end, sizeof(uint32_t) * nnz);
        }
    }
    lk.lock();
    g->pending -= 1;
    cv_copy.notify_all();
    if (out_ticket) *out_ticket = ticket;
    return OEM_OK;
}

extern "C" int oem_cells_stream_push(oem_cells_stream *s, const uint64_t *row_ptr, const uint32_t *tid, const float *as_prob,
                                     const uint32_t *aln_start, const uint32_t *aln_end, uint64_t n_reads, uint64_t nnz,
                                     uint64_t *out_ticket)
{
    const char *who = "oem_cells_stream_push";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    // the cell's own checks, on the calling thread, before the session is touched
    if (!row_ptr) return fail(OEM_ERR_ARG, "%s: row_ptr is NULL", who);
    if (nnz > 0 && (!tid || !as_prob)) return fail(OEM_ERR_ARG, "%s: tid/as_prob is NULL", who);
    if (s->o.coverage && nnz > 0 && (!aln_start || !aln_end))
        return fail(OEM_ERR_ARG, "%s: coverage = 1 needs aln_start and aln_end", who);
    if (n_reads >= (1ull << 32) || nnz >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: a cell needs fewer than 2^32 reads and alignments", who);
    try {
        OEM_TRY(validate_csr(row_ptr, tid, n_reads, nnz, s->o.n_txps));
    } catch (const std::exception &) {
        return fail(OEM_ERR_OOM, "%s: host allocation failed", who);
    }

    CellArrays a;
    a.rp = row_ptr;
    a.tid = tid;
    a.p = as_prob;
    a.start = aln_start;
    a.end = aln_end;
    return s->push_cell(who, false, a, n_reads, nnz, out_ticket);
}

extern "C" int oem_cells_stream_set_filters(oem_cells_stream *s, const oem_filters *filters, const uint64_t *txp_len)
{
    OEM_API_BEGIN
    const char *who = "oem_cells_stream_set_filters";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    if (!filters || !txp_len) return fail(OEM_ERR_ARG, "%s: NULL argument", who);
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->finish_called || s->cancel) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
    if (s->next_ticket || s->pushes_in_flight || s->open) return fail(OEM_ERR_STATE, "%s: a cell has been pushed already", who);
    OEM_TRY(records_filter_setup(who, filters, txp_len, s->o.n_txps, &s->rf));
    s->records_mode = true; // (no arena exists yet: the first push makes the first one, in the records layout)
    return OEM_OK;
    OEM_API_END("oem_cells_stream_set_filters")
}

extern "C" int oem_cells_stream_push_records(oem_cells_stream *s, const oem_aln_record *records, const uint64_t *group_off,
                                             uint64_t n_groups, uint64_t *out_ticket)
{
    const char *who = "oem_cells_stream_push_records";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    // the cell's own checks, on the calling thread, before the session is touched
    OEM_TRY(check_group_off(who, records, group_off, n_groups));
    if (n_groups >= 0x7fffffffull || group_off[n_groups] >= (1ull << 32))
        return fail(OEM_ERR_ARG, "%s: a cell needs fewer than 2^31 - 1 reads and 2^32 records", who);
    CellArrays a;
    a.rp = group_off;
    a.rec = records;
    return s->push_cell(who, true, a, n_groups, group_off[n_groups], out_ticket);
}

// oem_cells_stream_set_barcodes and oem_cells_stream_set_barcodes_any_order: the same preconditions, the same session
// behind them; any_order chooses the rule the batches' cells are found by.
static int set_barcodes(oem_cells_stream *s, const char *who, uint32_t mode, bool any_order)
{
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    if (mode != kCollateSort && mode != kCollateAdjacent)
        return fail(OEM_ERR_ARG, "%s: mode must be OEM_COLLATE_SORT or OEM_COLLATE_ADJACENT", who);
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->finish_called || s->cancel) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
    if (s->bc) return fail(OEM_ERR_STATE, "%s: the session is a barcoded session already", who);
    if (!s->records_mode) return fail(OEM_ERR_STATE, "%s: not a records session (oem_cells_stream_set_filters)", who);
    if (s->next_ticket || s->pushes_in_flight || s->open) return fail(OEM_ERR_STATE, "%s: a cell has been pushed already", who);
    BarcodesEnv env;
    env.n_txps = s->o.n_txps;
    env.device = s->o.device;
    env.max_iter = s->o.max_iter;
    env.conv_thresh = s->o.conv_thresh;
    env.cov = s->o.coverage ? &s->cov : nullptr;
    env.rf = &s->rf;
    env.group_nnz = s->group_nnz;
    env.group_cells = s->group_cells;
    env.max_staged = s->max_staged;
    env.mode = mode;
    env.submit = [s](StreamGroupRun run) { // the group's place in the result is its place in this order
        std::unique_ptr<Group> g(new Group());
        g->dev_run = std::move(run);
        std::lock_guard<std::mutex> lk2(s->mu);
        g->index = s->results.size();
        s->results.emplace_back();
        s->queue.push_back(std::move(g));
        s->cv_work.notify_one();
    };
    env.set_sticky = [s](int rc, const char *msg) {
        std::lock_guard<std::mutex> lk2(s->mu);
        s->set_sticky(rc, msg);
    };
    env.sticky = [s](std::string *msg) {
        std::lock_guard<std::mutex> lk2(s->mu);
        if (s->sticky_rc != OEM_OK) *msg = s->sticky_msg;
        return s->sticky_rc;
    };
    return barcodes_stream_create(env, any_order, &s->bc);
}

extern "C" int oem_cells_stream_set_barcodes(oem_cells_stream *s, uint32_t mode)
{
    OEM_API_BEGIN
    return set_barcodes(s, "oem_cells_stream_set_barcodes", mode, false);
    OEM_API_END("oem_cells_stream_set_barcodes")
}

extern "C" int oem_cells_stream_set_barcodes_any_order(oem_cells_stream *s, uint32_t mode)
{
    OEM_API_BEGIN
    return set_barcodes(s, "oem_cells_stream_set_barcodes_any_order", mode, true);
    OEM_API_END("oem_cells_stream_set_barcodes_any_order")
}

extern "C" int oem_cells_stream_push_barcodes(oem_cells_stream *s, const oem_aln_record *records, uint64_t n_records,
                                              const uint8_t *barcodes, const uint64_t *barcode_off, const uint8_t *names,
                                              const uint64_t *name_off, const uint8_t *secondary, uint64_t *out_ticket)
{
    OEM_API_BEGIN
    const char *who = "oem_cells_stream_push_barcodes";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    if (!s->bc) return fail(OEM_ERR_STATE, "%s: not a barcoded session (oem_cells_stream_set_barcodes)", who);
    return barcodes_stream_push(s->bc, who, records, n_records, barcodes, barcode_off, names, name_off, secondary, false, nullptr, nullptr,
                                out_ticket);
    OEM_API_END("oem_cells_stream_push_barcodes")
}

// A UMI session (oem_collate.h, "UMIs in the sessions"): a barcoded session of either form whose batches bring one UMI
// per record; its groups are deduplicated behind their name collation (oem_cells_barcodes_stream.hip).
extern "C" int oem_cells_stream_set_umis(oem_cells_stream *s)
{
    OEM_API_BEGIN
    const char *who = "oem_cells_stream_set_umis";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->finish_called || s->cancel) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
        if (!s->bc) return fail(OEM_ERR_STATE, "%s: not a barcoded session (oem_cells_stream_set_barcodes)", who);
    }
    return barcodes_stream_set_umis(s->bc, who);
    OEM_API_END("oem_cells_stream_set_umis")
}

extern "C" int oem_cells_stream_push_barcodes_umis(oem_cells_stream *s, const oem_aln_record *records, uint64_t n_records,
                                                   const uint8_t *barcodes, const uint64_t *barcode_off, const uint8_t *names,
                                                   const uint64_t *name_off, const uint8_t *secondary, const uint8_t *umis,
                                                   const uint64_t *umi_off, uint64_t *out_ticket)
{
    OEM_API_BEGIN
    const char *who = "oem_cells_stream_push_barcodes_umis";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    if (!s->bc) return fail(OEM_ERR_STATE, "%s: not a barcoded session (oem_cells_stream_set_barcodes)", who);
    return barcodes_stream_push(s->bc, who, records, n_records, barcodes, barcode_off, names, name_off, secondary, true, umis, umi_off,
                                out_ticket);
    OEM_API_END("oem_cells_stream_push_barcodes_umis")
}

extern "C" int oem_cells_stream_umis_copy(const oem_cells_stream *s, uint64_t *out_cell_dups)
{
    const char *who = "oem_cells_stream_umis_copy";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    if (!s->bc) return fail(OEM_ERR_STATE, "%s: not a UMI session (oem_cells_stream_set_umis)", who);
    return barcodes_stream_umis_copy(s->bc, who, out_cell_dups);
}

// The UMI rule of a UMI session (oem_collate.h, "The UMI rule"): gene-aware keys and one-mismatch correction in every
// group's dedup_mark, as oem_em_run_cells_records_umis_rule_sparse has them.
extern "C" int oem_cells_stream_set_umi_rule(oem_cells_stream *s, const oem_umi_rule *rule)
{
    OEM_API_BEGIN
    const char *who = "oem_cells_stream_set_umi_rule";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->finish_called || s->cancel) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
        if (!s->bc) return fail(OEM_ERR_STATE, "%s: not a UMI session (oem_cells_stream_set_umis)", who);
    }
    return barcodes_stream_set_umi_rule(s->bc, who, rule);
    OEM_API_END("oem_cells_stream_set_umi_rule")
}

extern "C" int oem_cells_stream_umi_rule_copy(const oem_cells_stream *s, uint64_t *out_cell_corrected)
{
    const char *who = "oem_cells_stream_umi_rule_copy";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    if (!s->bc) return fail(OEM_ERR_STATE, "%s: not a UMI session under a rule with correct (oem_cells_stream_set_umi_rule)", who);
    return barcodes_stream_umi_rule_copy(s->bc, who, out_cell_corrected);
}

// The barcode rule of an any-order barcoded session (oem_barcode_correct.h, "The rule in a session"): raw barcodes
// corrected against a whitelist batch by batch, as oem_em_run_cells_records_whitelist_sparse corrects them in one call.
extern "C" int oem_cells_stream_set_whitelist(oem_cells_stream *s, const oem_barcode_rule *rule)
{
    OEM_API_BEGIN
    const char *who = "oem_cells_stream_set_whitelist";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->finish_called || s->cancel) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
        if (!s->bc) return fail(OEM_ERR_STATE, "%s: not an any-order barcoded session (oem_cells_stream_set_barcodes_any_order)", who);
    }
    return barcodes_stream_set_whitelist(s->bc, who, rule);
    OEM_API_END("oem_cells_stream_set_whitelist")
}

extern "C" int oem_cells_stream_whitelist_copy(const oem_cells_stream *s, uint32_t *out_cell_wl_id, uint64_t *out_cell_bc_corrected,
                                               uint64_t *out_counts)
{
    const char *who = "oem_cells_stream_whitelist_copy";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    if (!s->bc) return fail(OEM_ERR_STATE, "%s: not a whitelist session (oem_cells_stream_set_whitelist)", who);
    return barcodes_stream_whitelist_copy(s->bc, who, out_cell_wl_id, out_cell_bc_corrected, out_counts);
}

extern "C" int oem_cells_stream_barcodes_dims(const oem_cells_stream *s, uint64_t *n_cells, uint64_t *n_survivors, uint64_t *n_groups,
                                              uint64_t *barcode_bytes, uint64_t *n_unmapped)
{
    const char *who = "oem_cells_stream_barcodes_dims";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    if (!s->bc) return fail(OEM_ERR_STATE, "%s: not a barcoded session (oem_cells_stream_set_barcodes)", who);
    return barcodes_stream_dims(s->bc, who, n_cells, n_survivors, n_groups, barcode_bytes, n_unmapped);
}

extern "C" int oem_cells_stream_barcodes_copy(const oem_cells_stream *s, uint8_t *out_barcodes, uint64_t *out_barcode_off,
                                              uint64_t *out_cell_rec_off, uint64_t *out_order, uint64_t *out_group_off,
                                              uint64_t *out_cell_group_off, uint32_t *out_kept)
{
    const char *who = "oem_cells_stream_barcodes_copy";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    if (!s->bc) return fail(OEM_ERR_STATE, "%s: not a barcoded session (oem_cells_stream_set_barcodes)", who);
    return barcodes_stream_copy(s->bc, who, out_barcodes, out_barcode_off, out_cell_rec_off, out_order, out_group_off,
                                out_cell_group_off, out_kept);
}

extern "C" int oem_cells_stream_finish(oem_cells_stream *s, oem_cells_result **out)
{
    OEM_API_BEGIN
    const char *who = "oem_cells_stream_finish";
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->finish_called) return fail(OEM_ERR_STATE, "%s: the session is finished already", who);
        if (s->pushes_in_flight || (s->bc && barcodes_stream_push_in_flight(s->bc))) return fail(OEM_ERR_STATE, "%s: a push is in flight", who);
        s->finish_called = true;
        s->close_open();
        if (!s->bc) s->stop = true;
    }
    int bc_rc = OEM_OK;
    std::string bc_msg;
    if (s->bc) { // the staged batches are parsed, the open cell closes, the last groups go to the workers
        bc_rc = barcodes_stream_close(s->bc, who);
        if (bc_rc != OEM_OK) bc_msg = last_error_text();
        std::lock_guard<std::mutex> lk(s->mu);
        s->stop = true;
    }
    s->cv_work.notify_all();
    for (auto &t : s->workers)
        if (t.joinable()) t.join();
    if (s->sticky_rc != OEM_OK) return fail(s->sticky_rc, "%s", s->sticky_msg.c_str());
    if (bc_rc != OEM_OK) return fail(bc_rc, "%s", bc_msg.c_str());
    uint64_t n_cells = s->next_ticket;
    if (s->bc) {
        OEM_TRY(barcodes_stream_assemble(s->bc, who));
        OEM_TRY(barcodes_stream_dims(s->bc, who, &n_cells, nullptr, nullptr, nullptr, nullptr));
    }
    std::unique_ptr<oem_cells_result> r(new oem_cells_result());
    r->n_cells = (uint32_t)n_cells;
    r->infos.reserve(r->n_cells);
    std::vector<SparseBlock> blocks;
    blocks.reserve(s->results.size());
    r->from_records = s->records_mode;
    for (GroupResult &gr : s->results) { // group order is ticket order
        r->infos.insert(r->infos.end(), gr.infos.begin(), gr.infos.end());
        r->discard.insert(r->discard.end(), gr.tables.begin(), gr.tables.end());
        blocks.push_back(std::move(gr.blk));
    }
    s->results.clear();
    if (r->infos.size() != r->n_cells) return fail(OEM_ERR_STATE, "%s: the groups' results cover %zu of %u cells", who, r->infos.size(), r->n_cells);
    OEM_TRY(cells_result_from_blocks(who, blocks, r.get()));
    *out = r.release();
    return OEM_OK;
    OEM_API_END("oem_cells_stream_finish")
}

extern "C" int oem_cells_stream_info(const oem_cells_stream *s, uint32_t key, uint64_t *value)
{
    if (!s || !value) return fail(OEM_ERR_ARG, "oem_cells_stream_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mu);
    uint64_t bc_batches = 0, bc_records = 0, bc_blocked_us = 0, bc_arena = 0, bc_misses = 0, bc_slots = 0;
    if (s->bc) barcodes_stream_counts(s->bc, &bc_batches, &bc_records, &bc_blocked_us);
    if (s->bc) barcodes_stream_table_info(s->bc, &bc_arena, &bc_misses, &bc_slots);
    uint64_t dup_reads = 0, dup_records = 0, corrected_reads = 0;
    if (s->bc) barcodes_stream_umi_info(s->bc, &dup_reads, &dup_records, &corrected_reads);
    uint64_t bc_rejected = 0, bc_deferred = 0;
    if (s->bc) barcodes_stream_whitelist_info(s->bc, &bc_rejected, &bc_deferred);
    switch (key) {
    case OEM_CELLS_STREAM_INFO_BARCODE_REJECTED: *value = bc_rejected; break; // (a whitelist session; 0 otherwise)
    case OEM_CELLS_STREAM_INFO_BARCODE_DEFERRED: *value = bc_deferred; break;
    case OEM_CELLS_STREAM_INFO_UMI_CORRECTED_READS: *value = corrected_reads; break; // (under a rule with correct; 0 otherwise)
    case OEM_CELLS_STREAM_INFO_UMI_DUP_READS: *value = dup_reads; break; // (a UMI session; 0 otherwise)
    case OEM_CELLS_STREAM_INFO_UMI_DUP_RECORDS: *value = dup_records; break;
    case OEM_CELLS_STREAM_INFO_ARENA_BYTES: *value = bc_arena; break; // (an any-order barcoded session; 0 otherwise)
    case OEM_CELLS_STREAM_INFO_BARCODE_MISSES: *value = bc_misses; break;
    case OEM_CELLS_STREAM_INFO_BARCODE_TABLE_SLOTS: *value = bc_slots; break;
    case OEM_CELLS_STREAM_INFO_CELLS: *value = s->bc ? bc_batches : s->next_ticket; break; // (a barcoded session: batches)
    case OEM_CELLS_STREAM_INFO_ALIGNMENTS: *value = s->bc ? bc_records : s->total_nnz; break;
    case OEM_CELLS_STREAM_INFO_GROUPS: *value = s->groups_started; break;
    case OEM_CELLS_STREAM_INFO_GROUPS_BEFORE_FINISH: *value = s->groups_before_finish; break;
    case OEM_CELLS_STREAM_INFO_BLOCKED_US: *value = s->blocked_us + bc_blocked_us; break; // (a barcoded session: its staging queue's)
    case OEM_CELLS_STREAM_INFO_GROUPS_BATCHED: *value = s->groups_batched; break;
    default: return fail(OEM_ERR_ARG, "oem_cells_stream_info: unknown key %u", key);
    }
    return OEM_OK;
}

extern "C" void oem_cells_stream_destroy(oem_cells_stream *s)
{
    if (!s) return;
    if (s->bc) barcodes_stream_cancel(s->bc); // (nothing more is parsed or handed to the workers)
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (!s->finish_called) s->cancel = true; // queued groups are dropped; a group on the device runs to its end
        s->finish_called = true;
        if (s->open) s->queue.push_back(std::move(s->open)); // (skipped by the worker that takes it)
        s->stop = true;
    }
    s->cv_work.notify_all();
    s->cv_space.notify_all();
    for (auto &t : s->workers)
        if (t.joinable()) t.join();
    (void)hipSetDevice(s->o.device); // the coverage tables and the pinned arenas are released on their device
    barcodes_stream_destroy(s->bc);
    delete s;
}
