// oem_records_stream.hip -- the bulk records session (oem_records_stream_*): oem_store_create_records
// for a caller that never holds all records at once (parse_alignments, alignment_parser.rs:301-437, adds group by
// group; the raw-read drivers of bulk.rs:364-682 hand chunks from mapper threads to a consumer).
//
//   push      checks the batch on the calling thread, waits for room in the staging budget, takes the batch's ticket under
//             the session lock and copies group offsets and records into a page-locked arena outside it: the staging
//             copies of several pushing threads run side by side, where the one call has one thread for all of them.
//             Arenas are reused from batch to batch (page-locking memory costs more than filling it).
//   worker    one thread takes the batches in ticket order and runs the pass of the one call on each of them
//             (filter_device with pinned_src: the uploads straight from the arena on two lanes, k_filter_measure behind
//             each chunk, the scans, k_filter_emit), with base 0.  What stays is the batch's PIECE: its CSR with u32 row
//             pointers from 0, its kept counts and its discard counters; coordinates and strand only under a coverage
//             model.  The batch's device records are freed inside the pass, its arena goes back to the pool.  The
//             fallbacks are the one call's, per batch: the host loop takes a batch with a score beyond +-2^24, or every
//             batch when score_prob_denom has no table, and its piece is uploaded.
//   finish    joins the worker, scans the pieces' sizes into per-piece row, alignment and group bases and launches
//             k_stream_concat once over all arrays of all pieces: the result is the FilterResult the one call's pass
//             would have left, and filter_result_to_store makes the store of it.  The pieces are freed after the join.
//
// The batch type is oem_aln_record throughout; a session over projected records would template Batch and run_batch on
// the record type, as filter_upload_measure is.
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

#include "oem_filter_device.h"

namespace oem {
namespace {

// Default of oem_records_stream_opts.max_staged_records, from the sweep of scripts/records_stream_bench.py
// (profiles/records_stream_bench.json): 8 Mi records (320 MiB of page-locked staging) with batches
// of 256 Ki groups gave 0.205 - 0.226 s for 1, 2, 4 and 8 pushing threads alike; 2 Mi starves the device worker (0.32 -
// 0.39 s), 32 Mi page-locks more memory than it saves (0.23 - 0.30 s) except for one thread pushing batches of 1 Mi
// groups (0.198 s, the best point of the sweep).  A batch larger than the budget is pushed and filtered in turn, with no
// overlap at all: keep batches under a quarter of it.
constexpr uint64_t kDefaultMaxStaged = 8ull << 20;
constexpr int kPoolArenas = 16; // idle arenas kept for reuse
constexpr int kCT = 256;

thread_local float g_join_ms = 0.f;

// One array of one piece on its way into the joined result: n_bytes from src to dst, as u32 elements with `add` added
// to each (elem 4: row pointers get the piece's alignment base, the other arrays 0) or as bytes (elem 1: strand).
// The job's workgroups are first_block .. of the one launch.
struct ConcatJob {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t n_bytes;
    uint64_t first_block;
    uint32_t add;
    uint32_t elem;
};

// The split of a job into a head (up to the destination's first 16-byte boundary), 16-byte body units and a tail.  A
// byte job whose source is not 4-byte aligned where the body starts assembles each unit from five aligned words, the
// last of which may reach 3 bytes past the unit: the body ends 4 bytes early so that no load passes the source's end.
struct ConcatSplit {
    uint64_t head, n_body;
    uint32_t rel; // the source's offset from 16-byte alignment where the body starts
};
__host__ __device__ inline ConcatSplit concat_split(const ConcatJob &j)
{
    ConcatSplit s;
    s.head = (16 - ((uintptr_t)j.dst & 15)) & 15;
    if (s.head > j.n_bytes) s.head = j.n_bytes;
    s.rel = (uint32_t)(((uintptr_t)j.src + s.head) & 15);
    const uint64_t rest = j.n_bytes - s.head, slack = (s.rel & 3) ? 4 : 0;
    s.n_body = rest >= slack ? (rest - slack) / 16 : 0;
    return s;
}
// units of a job: its body units plus one lane for head and tail
inline uint64_t concat_blocks(const ConcatJob &j) { return (concat_split(j).n_body + 1 + kCT - 1) / kCT; }

// The join of a session's pieces, every array of every piece in one launch.  A workgroup finds its job by binary search
// over the jobs' first workgroups (uniform: scalar loads); a lane moves 16 bytes with one aligned 16-byte store, so a
// wavefront writes 1 KiB contiguously.  The piece's alignment base is arbitrary, so source and destination are in
// general not aligned alike: the load is one 16-byte load where they are, four 4-byte loads where they differ by a
// multiple of 4 (every u32 array; consecutive lanes still read consecutive addresses), and five aligned words shifted
// into place for a byte array at an odd offset.  The lane after the body copies head and tail element by element.
__global__ __launch_bounds__(kCT) void k_stream_concat(const ConcatJob *__restrict__ jobs, uint32_t n_jobs)
{
    uint32_t a = 0, b = n_jobs;
    while (b - a > 1) {
        const uint32_t m = (a + b) >> 1;
        if (jobs[m].first_block <= blockIdx.x) a = m;
        else b = m;
    }
    const ConcatJob j = jobs[a];
    const ConcatSplit sp = concat_split(j);
    const uint64_t u = (uint64_t)(blockIdx.x - j.first_block) * kCT + threadIdx.x;
    if (u < sp.n_body) {
        const uint8_t *s = j.src + sp.head + 16 * u;
        uint4 v;
        if (sp.rel == 0) {
            v = *(const uint4 *)s;
        } else if ((sp.rel & 3) == 0) {
            const uint32_t *s4 = (const uint32_t *)s;
            v = make_uint4(s4[0], s4[1], s4[2], s4[3]);
        } else {
            const uint32_t r = sp.rel & 3, lo = 8 * r, hi = 32 - lo;
            const uint32_t *w = (const uint32_t *)(s - r);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            v = make_uint4((w0 >> lo) | (w1 << hi), (w1 >> lo) | (w2 << hi), (w2 >> lo) | (w3 << hi), (w3 >> lo) | (w4 << hi));
        }
        v.x += j.add; // (0 for everything but row pointers)
        v.y += j.add;
        v.z += j.add;
        v.w += j.add;
        *(uint4 *)(j.dst + sp.head + 16 * u) = v;
    } else if (u == sp.n_body) {
        const uint64_t t0 = sp.head + 16 * sp.n_body;
        if (j.elem == 4) {
            for (uint64_t i = 0; i < sp.head; i += 4) *(uint32_t *)(j.dst + i) = *(const uint32_t *)(j.src + i) + j.add;
            for (uint64_t i = t0; i < j.n_bytes; i += 4) *(uint32_t *)(j.dst + i) = *(const uint32_t *)(j.src + i) + j.add;
        } else {
            for (uint64_t i = 0; i < sp.head; ++i) j.dst[i] = j.src[i];
            for (uint64_t i = t0; i < j.n_bytes; ++i) j.dst[i] = j.src[i];
        }
    }
}

// page-locked (or, when that allocation fails, pageable) host memory of one batch: its group offsets, then its records
struct Arena {
    void *p = nullptr;
    size_t bytes = 0;
    bool pinned = false;
};
void arena_free(Arena &a)
{
    if (a.pinned) (void)hipHostFree(a.p);
    else free(a.p);
    a = Arena();
}

struct Batch {
    uint64_t ticket = 0, n_groups = 0, n_records = 0;
    Arena mem;          // (none for a batch without groups)
    bool ready = false; // the pushing thread has finished its copy
    Batch() = default;
    Batch(const Batch &) = delete;
    Batch &operator=(const Batch &) = delete;
    ~Batch() { if (mem.p) arena_free(mem); }
    const uint64_t *group_off() const { return (const uint64_t *)mem.p; }
    static size_t records_at(uint64_t n_groups) { return (sizeof(uint64_t) * (n_groups + 1) + 63) & ~(size_t)63; }
    const oem_aln_record *records() const { return (const oem_aln_record *)((const char *)mem.p + records_at(n_groups)); }
};

// What a batch leaves on the device: r.row_ptr32 (n_rows + 1, from 0), r.tid, r.as_prob, with a model r.start / r.end /
// r.strand, r.n_kept (n_groups + 1) and r.dt.  A batch without groups leaves no arrays.
struct Piece {
    FilterResult r;
    uint64_t n_groups = 0;
};

} // namespace
} // namespace oem

using namespace oem;

struct oem_records_stream {
    oem_records_stream_opts o;
    oem_filters f;
    std::vector<uint64_t> txp_len;
    std::vector<float> tab; // filter_prob_table of f.score_prob_denom
    bool host_only = false; // ... or there is none: the host loop takes every batch
    uint64_t max_staged = 0;

    mutable std::mutex mu;
    std::condition_variable cv_work, cv_space;
    std::deque<std::unique_ptr<Batch>> queue; // ticket order
    std::vector<Arena> pool;
    std::vector<std::unique_ptr<Piece>> pieces; // by ticket
    uint64_t next_ticket = 0, total_groups = 0, total_records = 0, staged_records = 0, total_kept = 0;
    uint64_t before_finish = 0, blocked_us = 0, host_batches = 0;
    int pushes_in_flight = 0;
    bool finish_called = false, stop = false, cancel = false;
    int sticky_rc = OEM_OK;
    std::string sticky_msg;
    std::thread worker;

    ~oem_records_stream()
    {
        for (Arena &a : pool) arena_free(a);
    }
    void set_sticky(int rc, const char *msg) // (mu held)
    {
        if (sticky_rc != OEM_OK) return;
        sticky_rc = rc;
        sticky_msg = msg;
    }
    // (mu held) the smallest idle arena that holds `bytes`, or an empty one
    Arena take_arena(size_t bytes)
    {
        size_t best = pool.size();
        for (size_t k = 0; k < pool.size(); ++k)
            if (pool[k].bytes >= bytes && (best == pool.size() || pool[k].bytes < pool[best].bytes)) best = k;
        if (best == pool.size()) return Arena();
        Arena a = pool[best];
        pool.erase(pool.begin() + best);
        return a;
    }
    void give_arena(Arena &a) // (mu held)
    {
        if (!a.p) return;
        if (pool.size() >= (size_t)kPoolArenas) { // the smallest one goes
            size_t least = 0;
            for (size_t k = 1; k < pool.size(); ++k)
                if (pool[k].bytes < pool[least].bytes) least = k;
            if (pool[least].bytes < a.bytes) std::swap(pool[least], a);
            arena_free(a);
            return;
        }
        pool.push_back(a);
        a = Arena();
    }

    int run_batch(const Batch &b, Piece *out, bool *host);
    int host_piece(const Batch &b, const char *who, Piece *out);
    void work();
    int join(const char *who, FilterResult *out, uint64_t *n_groups);
    int finish_begin(const char *who);
};

// The host loop on one batch (a fresh builder: bases 0), and its arrays uploaded as the piece.
int oem_records_stream::host_piece(const Batch &b, const char *who, Piece *out)
{
    FilterResult &r = out->r;
    r.row_ptr32.reset(); // (a device pass that met a big score has left n_kept behind)
    r.n_kept.reset();
    oem_builder hb;
    hb.f = f;
    hb.txp_len = txp_len;
    std::vector<uint32_t> kept(b.n_groups + 1, 0);
    OEM_TRY(add_groups_host(&hb, b.records(), b.group_off(), b.n_groups, kept.data(), who));
    const uint64_t nnz = hb.tid.size(), n_rows = hb.row_ptr.size() - 1;
    if (nnz >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: a resident store needs fewer than 2^32 alignments", who);
    std::vector<uint32_t> rp32(hb.row_ptr.begin(), hb.row_ptr.end());
    auto up = [&](auto *dbuf, const auto *src, uint64_t n) -> int {
        OEM_TRY(dev_alloc(&dbuf->p, n, nullptr));
        if (n) OEM_HIP(hipMemcpy(dbuf->p, src, sizeof(*src) * n, hipMemcpyHostToDevice));
        return OEM_OK;
    };
    OEM_TRY(up(&r.row_ptr32, rp32.data(), n_rows + 1));
    OEM_TRY(up(&r.n_kept, kept.data(), b.n_groups + 1));
    OEM_TRY(up(&r.tid, hb.tid.data(), nnz));
    OEM_TRY(up(&r.as_prob, hb.as_prob.data(), nnz));
    if (o.model >= 0) {
        OEM_TRY(up(&r.start, hb.start.data(), nnz));
        OEM_TRY(up(&r.end, hb.end.data(), nnz));
        OEM_TRY(up(&r.strand, hb.strand.data(), nnz));
    }
    r.n_rows = n_rows;
    r.nnz = nnz;
    r.dt = hb.dt;
    r.host_rerun = false;
    return OEM_OK;
}

int oem_records_stream::run_batch(const Batch &b, Piece *out, bool *host)
{
    out->n_groups = b.n_groups;
    if (b.n_groups == 0) return OEM_OK;
    char who[64];
    snprintf(who, sizeof who, "oem_records_stream: ticket %llu", (unsigned long long)b.ticket);
    if (!host_only) {
        OEM_TRY(filter_device(who, f, txp_len.data(), o.n_txps, tab, b.records(), b.group_off(), b.n_groups, 0, o.model >= 0, true,
                              &out->r, nullptr, b.mem.pinned));
        out->r.txp_len.reset(); // (the join uploads the lengths once)
        if (!out->r.host_rerun) return OEM_OK;
    }
    *host = true;
    return host_piece(b, who, out);
}

void oem_records_stream::work()
{
    const bool dev_ok = hipSetDevice(o.device) == hipSuccess;
    for (;;) {
        std::unique_ptr<Batch> b;
        bool skip;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv_work.wait(lk, [&] { return (!queue.empty() && queue.front()->ready) || (stop && queue.empty()); });
            if (queue.empty()) break;
            b = std::move(queue.front());
            queue.pop_front();
            if (!dev_ok) set_sticky(OEM_ERR_HIP, "oem_records_stream: the device worker could not select its device");
            skip = cancel || sticky_rc != OEM_OK;
            if (!skip && !finish_called) ++before_finish;
        }
        std::unique_ptr<Piece> piece;
        bool host = false;
        int rc = OEM_OK;
        std::string msg;
        if (!skip) {
            try {
                piece.reset(new Piece());
                rc = run_batch(*b, piece.get(), &host);
            } catch (const std::bad_alloc &) {
                rc = fail(OEM_ERR_OOM, "oem_records_stream: host allocation failed in the device worker");
            } catch (const std::exception &e) {
                rc = fail(OEM_ERR_STATE, "oem_records_stream: %s", e.what());
            }
            if (rc != OEM_OK) {
                msg = last_error_text(); // (the message is thread-local)
                piece.reset();
            }
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            staged_records -= b->n_records;
            give_arena(b->mem);
            if (rc != OEM_OK) {
                set_sticky(rc, msg.c_str());
            } else if (!skip) {
                total_kept += piece->r.nnz;
                if (host) ++host_batches;
                if (total_kept >= (1ull << 32))
                    set_sticky(OEM_ERR_ARG, "oem_records_stream: 2^32 or more alignments are kept; a resident store needs fewer");
                pieces[b->ticket] = std::move(piece);
            }
        }
        cv_space.notify_all();
    }
}

// The pieces, in ticket order, as the one FilterResult the one call's pass leaves: bases from a scan over the pieces'
// sizes, then k_stream_concat.  The pieces are freed.
int oem_records_stream::join(const char *who, FilterResult *out, uint64_t *n_groups)
{
    g_join_ms = 0.f;
    const bool coords = o.model >= 0;
    uint64_t R = 0, A = 0, G = 0;
    for (const auto &p : pieces) {
        if (!p) return fail(OEM_ERR_STATE, "%s: a batch has left no piece", who);
        R += p->r.n_rows;
        A += p->r.nnz;
        G += p->n_groups;
    }
    if (A >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: %llu alignments are kept; a resident store needs fewer than 2^32", who, (unsigned long long)A);
    out->n_rows = R;
    out->nnz = A;
    OEM_TRY(dev_alloc(&out->row_ptr32.p, R + 1, nullptr));
    OEM_TRY(dev_alloc(&out->n_kept.p, G + 1, nullptr));
    OEM_TRY(dev_alloc(&out->tid.p, A, nullptr));
    OEM_TRY(dev_alloc(&out->as_prob.p, A, nullptr));
    if (coords) {
        OEM_TRY(dev_alloc(&out->start.p, A, nullptr));
        OEM_TRY(dev_alloc(&out->end.p, A, nullptr));
        OEM_TRY(dev_alloc(&out->strand.p, A, nullptr));
    }
    OEM_TRY(dev_alloc(&out->txp_len.p, o.n_txps, nullptr));
    OEM_HIP(hipMemcpy(out->txp_len.p, txp_len.data(), sizeof(uint64_t) * o.n_txps, hipMemcpyHostToDevice));
    OEM_HIP(hipMemset(out->row_ptr32.p, 0, sizeof(uint32_t)));

    std::vector<ConcatJob> jobs;
    uint64_t n_blocks = 0;
    auto add_job = [&](const void *src, void *dst, uint64_t n, uint32_t elem, uint32_t add) {
        if (n == 0) return;
        ConcatJob j{(const uint8_t *)src, (uint8_t *)dst, n * elem, n_blocks, add, elem};
        n_blocks += concat_blocks(j);
        jobs.push_back(j);
    };
    uint64_t *sum = &out->dt.discard_5p;
    uint64_t r0 = 0, a0 = 0, g0 = 0; // the piece's row, alignment and group base
    for (const auto &p : pieces) {
        const FilterResult &r = p->r;
        add_job(r.n_kept.p, out->n_kept.p + g0, p->n_groups, 4, 0);
        add_job(r.row_ptr32.p + 1, out->row_ptr32.p + r0 + 1, r.n_rows, 4, (uint32_t)a0);
        add_job(r.tid.p, out->tid.p + a0, r.nnz, 4, 0);
        add_job(r.as_prob.p, out->as_prob.p + a0, r.nnz, 4, 0);
        if (coords) {
            add_job(r.start.p, out->start.p + a0, r.nnz, 4, 0);
            add_job(r.end.p, out->end.p + a0, r.nnz, 4, 0);
            add_job(r.strand.p, out->strand.p + a0, r.nnz, 1, 0);
        }
        for (int k = 0; k < kFilterCounters; ++k) sum[k] += (&r.dt.discard_5p)[k];
        r0 += r.n_rows;
        a0 += r.nnz;
        g0 += p->n_groups;
    }
    if (n_blocks > 0x7fffffffull) return fail(OEM_ERR_ARG, "%s: the join needs %llu workgroups", who, (unsigned long long)n_blocks);
    if (!jobs.empty()) {
        DevBuf<ConcatJob> d_jobs;
        Event ev[2];
        OEM_TRY(dev_alloc(&d_jobs.p, jobs.size(), nullptr));
        OEM_HIP(hipMemcpy(d_jobs.p, jobs.data(), sizeof(ConcatJob) * jobs.size(), hipMemcpyHostToDevice));
        for (auto &e : ev) OEM_HIP(hipEventCreate(&e.e));
        OEM_HIP(hipEventRecord(ev[0].e, nullptr));
        hipLaunchKernelGGL(k_stream_concat, dim3((uint32_t)n_blocks), dim3(kCT), 0, nullptr, d_jobs.p, (uint32_t)jobs.size());
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipEventRecord(ev[1].e, nullptr));
        OEM_HIP(hipStreamSynchronize(nullptr));
        OEM_HIP(hipEventElapsedTime(&g_join_ms, ev[0].e, ev[1].e));
    }
    pieces.clear();
    *n_groups = G;
    return OEM_OK;
}

// What finish does before the join: the state checks, then the worker drains the queue and is joined.
int oem_records_stream::finish_begin(const char *who)
{
    {
        std::lock_guard<std::mutex> lk(mu);
        if (finish_called) return fail(OEM_ERR_STATE, "%s: the session is finished already", who);
        if (pushes_in_flight) return fail(OEM_ERR_STATE, "%s: a push is in flight", who);
        finish_called = true;
        stop = true;
    }
    cv_work.notify_all();
    if (worker.joinable()) worker.join();
    if (sticky_rc != OEM_OK) return fail(sticky_rc, "%s", sticky_msg.c_str());
    OEM_HIP(hipSetDevice(o.device));
    return OEM_OK;
}

extern "C" int oem_records_stream_create(const oem_records_stream_opts *opts, const oem_filters *filters, const uint64_t *txp_len,
                                         oem_records_stream **out)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_create";
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (!opts) return fail(OEM_ERR_ARG, "%s: opts is NULL", who);
    OEM_TRY(check_store_from_records(who, filters, txp_len, opts->n_txps, opts->bin_width, opts->model, nullptr));
    for (uint32_t r : opts->reserved)
        if (r) return fail(OEM_ERR_ARG, "%s: a reserved word is not 0", who);
    OEM_TRY(ensure_device(opts->device));
    std::unique_ptr<oem_records_stream> s(new oem_records_stream());
    s->o = *opts;
    s->f = *filters;
    s->txp_len.assign(txp_len, txp_len + opts->n_txps);
    s->host_only = !filter_prob_table(filters->score_prob_denom, s->tab);
    s->max_staged = opts->max_staged_records ? opts->max_staged_records : kDefaultMaxStaged;
    oem_records_stream *raw = s.get();
    raw->worker = std::thread([raw] { raw->work(); });
    *out = s.release();
    return OEM_OK;
    OEM_API_END("oem_records_stream_create")
}

extern "C" int oem_records_stream_push(oem_records_stream *s, const oem_aln_record *records, const uint64_t *group_off,
                                       uint64_t n_groups, uint64_t *out_ticket)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_push";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    // the batch's own checks, on the calling thread, before the session is touched
    OEM_TRY(check_group_off(who, records, group_off, n_groups));
    if (n_groups >= 0x7fffffffull) return fail(OEM_ERR_ARG, "%s: at most 2^31 - 2 groups per batch", who);
    const uint64_t n_records = group_off[n_groups];
    const size_t rec_at = Batch::records_at(n_groups), bytes = rec_at + sizeof(oem_aln_record) * n_records;

    Batch *b = nullptr;
    {
        std::unique_lock<std::mutex> lk(s->mu);
        ++s->pushes_in_flight;
        struct InFlight { // (mu is held whenever this scope is left)
            oem_records_stream *s;
            ~InFlight() { --s->pushes_in_flight; }
        } in_flight{s};
        for (;;) {
            if (s->finish_called || s->cancel) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
            if (s->sticky_rc != OEM_OK) return fail(s->sticky_rc, "%s", s->sticky_msg.c_str());
            if (s->staged_records == 0 || s->staged_records + n_records <= s->max_staged) break;
            const auto t0 = std::chrono::steady_clock::now();
            s->cv_space.wait(lk);
            s->blocked_us += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        }
        std::unique_ptr<Batch> nb(new Batch());
        s->pieces.reserve(s->pieces.size() + 1); // (so that taking the ticket below cannot throw half-way)
        nb->ticket = s->next_ticket;
        nb->n_groups = n_groups;
        nb->n_records = n_records;
        if (n_groups) nb->mem = s->take_arena(bytes);
        b = nb.get();
        s->queue.push_back(std::move(nb));
        s->pieces.emplace_back();
        ++s->next_ticket;
        s->total_groups += n_groups;
        s->total_records += n_records;
        s->staged_records += n_records;
        ++s->pushes_in_flight; // (the copy below: until the batch is ready)
    }
    // outside the lock: the arena, where the pool had none, and the copies.  The batch stays in the queue until it is
    // ready (the worker waits for that), so `b` is valid.
    bool oom = false;
    if (!b->mem.p && n_groups) {
        const size_t cap = bytes + bytes / 8 + 4096; // (batches of a run are of one size, more or less)
        if (hipSetDevice(s->o.device) == hipSuccess && hipHostMalloc(&b->mem.p, cap, hipHostMallocPortable) == hipSuccess) {
            b->mem.pinned = true;
        } else {
            (void)hipGetLastError();
            b->mem.p = malloc(cap);
            oom = !b->mem.p;
        }
        b->mem.bytes = cap;
    }
    if (b->mem.p) {
        std::memcpy(b->mem.p, group_off, sizeof(uint64_t) * (n_groups + 1));
        if (n_records) std::memcpy((char *)b->mem.p + rec_at, records, sizeof(oem_aln_record) * n_records);
    }
    const uint64_t ticket = b->ticket;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (oom) s->set_sticky(OEM_ERR_OOM, "oem_records_stream_push: host allocation of the staging memory failed");
        b->ready = true; // (after a failure the worker drops it: the session is stuck)
        --s->pushes_in_flight;
    }
    s->cv_work.notify_all();
    if (oom) return fail(OEM_ERR_OOM, "%s: host allocation of the staging memory failed", who);
    if (out_ticket) *out_ticket = ticket;
    return OEM_OK;
    OEM_API_END("oem_records_stream_push")
}

extern "C" int oem_records_stream_finish(oem_records_stream *s, const oem_store_opts *opts, uint32_t *out_kept,
                                         oem_discard_table *out_discard, oem_store **out)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_finish";
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    OEM_TRY(check_store_from_records(who, &s->f, s->txp_len.data(), s->o.n_txps, s->o.bin_width, s->o.model, opts));
    OEM_TRY(s->finish_begin(who));
    FilterResult r;
    uint64_t n_groups = 0;
    OEM_TRY(s->join(who, &r, &n_groups));
    return filter_result_to_store(who, r, s->o.n_txps, n_groups, s->o.bin_width, s->o.model, s->o.growth_rate, s->o.device, opts,
                                  out_kept, out_discard, out);
    OEM_API_END("oem_records_stream_finish")
}

namespace oem {

// The test-only library's oem_debug_records_stream_finish_csr: ends the session as finish does, but copies the joined
// CSR to the host instead of making a store of it.  dims3 = rows, alignments, groups, always; the arrays are copied
// when they fit caps3 (the same three; OEM_ERR_ARG otherwise).  start / end / strand are skipped without a model.
// *join_ms: k_stream_concat by HIP events.
int records_stream_finish_csr(oem_records_stream *s, uint64_t *dims3, const uint64_t *caps3, uint32_t *row_ptr, uint32_t *tid,
                              uint32_t *as_prob_bits, uint32_t *start, uint32_t *end, uint8_t *strand, uint32_t *kept,
                              oem_discard_table *dt, float *join_ms)
{
    const char *who = "oem_debug_records_stream_finish_csr";
    if (!s || !dims3 || !caps3) return fail(OEM_ERR_ARG, "%s: NULL argument", who);
    OEM_TRY(s->finish_begin(who));
    FilterResult r;
    uint64_t n_groups = 0;
    OEM_TRY(s->join(who, &r, &n_groups));
    dims3[0] = r.n_rows;
    dims3[1] = r.nnz;
    dims3[2] = n_groups;
    if (join_ms) *join_ms = g_join_ms;
    if (dt) *dt = r.dt;
    if (r.n_rows > caps3[0] || r.nnz > caps3[1] || n_groups > caps3[2])
        return fail(OEM_ERR_ARG, "%s: the result has %llu rows, %llu alignments, %llu groups", who, (unsigned long long)r.n_rows,
                    (unsigned long long)r.nnz, (unsigned long long)n_groups);
    auto back = [&](void *dst, const void *src, size_t bytes) -> int {
        if (dst && src && bytes) OEM_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return OEM_OK;
    };
    OEM_TRY(back(row_ptr, r.row_ptr32.p, sizeof(uint32_t) * (r.n_rows + 1)));
    OEM_TRY(back(tid, r.tid.p, sizeof(uint32_t) * r.nnz));
    OEM_TRY(back(as_prob_bits, r.as_prob.p, sizeof(float) * r.nnz));
    OEM_TRY(back(start, r.start.p, sizeof(uint32_t) * r.nnz));
    OEM_TRY(back(end, r.end.p, sizeof(uint32_t) * r.nnz));
    OEM_TRY(back(strand, r.strand.p, r.nnz));
    OEM_TRY(back(kept, r.n_kept.p, sizeof(uint32_t) * n_groups));
    return OEM_OK;
}

float records_stream_last_join_ms() { return g_join_ms; }

} // namespace oem

extern "C" int oem_records_stream_info(const oem_records_stream *s, uint32_t key, uint64_t *value)
{
    if (!s || !value) return fail(OEM_ERR_ARG, "oem_records_stream_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mu);
    switch (key) {
    case OEM_RECORDS_STREAM_INFO_BATCHES: *value = s->next_ticket; break;
    case OEM_RECORDS_STREAM_INFO_GROUPS: *value = s->total_groups; break;
    case OEM_RECORDS_STREAM_INFO_RECORDS: *value = s->total_records; break;
    case OEM_RECORDS_STREAM_INFO_BATCHES_BEFORE_FINISH: *value = s->before_finish; break;
    case OEM_RECORDS_STREAM_INFO_BLOCKED_US: *value = s->blocked_us; break;
    case OEM_RECORDS_STREAM_INFO_HOST_BATCHES: *value = s->host_batches; break;
    default: return fail(OEM_ERR_ARG, "oem_records_stream_info: unknown key %u", key);
    }
    return OEM_OK;
}

extern "C" void oem_records_stream_destroy(oem_records_stream *s)
{
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (!s->finish_called) s->cancel = true; // staged batches are dropped; the batch on the device runs to its end
        s->finish_called = true;
        s->stop = true;
    }
    s->cv_work.notify_all();
    s->cv_space.notify_all();
    if (s->worker.joinable()) s->worker.join();
    (void)hipSetDevice(s->o.device); // the pieces and the page-locked arenas are released on their device
    delete s;
}
