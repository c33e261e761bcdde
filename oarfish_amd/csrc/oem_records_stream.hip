// oem_records_stream.hip -- the bulk records session (oem_records_stream_*): oem_store_create_records
// for a caller that never holds all records at once (parse_alignments, alignment_parser.rs:301-437, adds group by
// group; the raw-read drivers of bulk.rs:364-682 hand chunks from mapper threads to a consumer).
//
//   push      checks the batch on the calling thread and hands it to the session's staging queue (oem_stage_queue.h: the
//             wait for room in the budget, the ticket, the reused page-locked arenas, the copies of several pushing
//             threads side by side, where the one call has one thread for all of them).  What is the session's own: the
//             order of its refusals (push_status), a batch's fields and its piece's slot (stage_batch), and the layout
//             the copy fills (Batch's accessors).
//   worker    the queue's one thread hands the batches over in ticket order (process); the pass of the one call runs on
//             each of them (filter_device with pinned_src: the uploads straight from the arena on two lanes, k_filter_measure behind
//             each chunk, the scans, k_filter_emit), with base 0.  What stays is the batch's PIECE: its CSR with u32 row
//             pointers from 0, its kept counts and its discard counters; coordinates and strand only under a coverage
//             model.  The batch's device records are freed inside the pass, its arena goes back to the pool.  The
//             fallbacks are the one call's, per batch: the host loop takes a batch with a score beyond +-2^24, or every
//             batch when score_prob_denom has no table, and its piece is uploaded.
//   finish    closes the queue (the worker runs what is staged and is joined), scans the pieces' sizes into per-piece row, alignment and group bases and launches
//             k_stream_concat once over all arrays of all pieces: the result is the FilterResult the one call's pass
//             would have left, and filter_result_to_store makes the store of it.  The pieces are freed after the join.
//
// The NAMES form (oem_records_stream_set_names; "the names session" below and in DESIGN.md section 5d) takes records and
// read names cut at any record positions: its worker parses each batch as oem_store_create_records_names does
// (oem_parse_device.h), carries the open read on the device from batch to batch, and its pieces hold the groups a batch
// CLOSED, with their group offsets and row names; finish joins those too.
//
// The PROJECTED form (oem_records_stream_set_projected; "the projected session" in DESIGN.md section 5d) takes batches
// of whole genome-mode groups with one read length per group.  Batch's accessors and run_batch are templates on the
// record type (oem_aln_record / oem_proj_record, 40 bytes both), as filter_upload_measure is: the projected batch's arena
// holds its read lengths behind its group offsets, its pass is proj_device with pinned_src, and its piece keeps, besides
// the CSR, the (index, f) list of the alignments whose expf the host has to supply (k_proj_collect).  finish joins the
// lists in the one k_stream_concat launch, the indices with the piece's alignment base added, and runs the host's expf
// and the scatter once, before filter_result_to_store.
//
// The SORTING NAMES form (oem_records_stream_set_sort; "the sorting names session" in DESIGN.md section 5d) takes records,
// read names and secondary flags in ANY order.  Nothing can be cut or filtered before the last record is in, so its
// worker only parses: each batch's survivors -- their records, dense names, flags and 64-bit session-global indices --
// are appended to a SurvivorArena (oem_dev_blob.h), which stays on the device and grows geometrically; finish runs the
// one call's tail (parse_tail, oem_parse_device.h) on the arena as on an uploaded input.
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "oem_dev_blob.h"
#include "oem_filter_device.h"
#include "oem_parse_device.h"
#include "oem_stage_queue.h"

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
// to each modulo 2^32 (elem 4: row pointers get the piece's alignment base, the other arrays 0), as u64 elements with
// the 64-bit `add` (elem 8: the names session's group offsets and row-name offsets get the piece's record and byte
// base) or as bytes (elem 1: strand, row names).  The job's workgroups are first_block .. of the one launch.
struct ConcatJob {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t n_bytes;
    uint64_t first_block;
    uint64_t add;
    uint32_t elem;
    uint32_t pad;
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
        if (j.elem == 8) { // (uniform per workgroup) two u64 elements: source and destination are 8-byte aligned, rel is 0 or 8
            const uint64_t e0 = (((uint64_t)v.y << 32) | v.x) + j.add, e1 = (((uint64_t)v.w << 32) | v.z) + j.add;
            v = make_uint4((uint32_t)e0, (uint32_t)(e0 >> 32), (uint32_t)e1, (uint32_t)(e1 >> 32));
        } else {
            const uint32_t add = (uint32_t)j.add; // (0 for everything but row pointers)
            v.x += add;
            v.y += add;
            v.z += add;
            v.w += add;
        }
        *(uint4 *)(j.dst + sp.head + 16 * u) = v;
    } else if (u == sp.n_body) {
        const uint64_t t0 = sp.head + 16 * sp.n_body;
        if (j.elem == 4) {
            const uint32_t add = (uint32_t)j.add;
            for (uint64_t i = 0; i < sp.head; i += 4) *(uint32_t *)(j.dst + i) = *(const uint32_t *)(j.src + i) + add;
            for (uint64_t i = t0; i < j.n_bytes; i += 4) *(uint32_t *)(j.dst + i) = *(const uint32_t *)(j.src + i) + add;
        } else if (j.elem == 8) {
            for (uint64_t i = 0; i < sp.head; i += 8) *(uint64_t *)(j.dst + i) = *(const uint64_t *)(j.src + i) + j.add;
            for (uint64_t i = t0; i < j.n_bytes; i += 8) *(uint64_t *)(j.dst + i) = *(const uint64_t *)(j.src + i) + j.add;
        } else {
            for (uint64_t i = 0; i < sp.head; ++i) j.dst[i] = j.src[i];
            for (uint64_t i = t0; i < j.n_bytes; ++i) j.dst[i] = j.src[i];
        }
    }
}

// A staged batch: in its arena (mem: none for a batch without groups, or without records in a names session) the group
// offsets, then the records.  rec_base is the session-global input index of its first record.
struct Batch : StageBatch {
    uint64_t n_groups = 0;
    // a names session's batch: no groups yet; the arena holds name_off (n_records + 1), the records and the name bytes
    bool named = false;
    bool projected = false; // a projected session's batch: whole groups of oem_proj_record with their read lengths
    bool sorting = false, has_sec = false; // a sorting names session's batch (named too); its n_records flags behind the names
    uint64_t name_bytes = 0; // name_off[n_records]
    const uint64_t *group_off() const { return (const uint64_t *)mem.p; }
    static size_t records_at(uint64_t n_groups) { return (sizeof(uint64_t) * (n_groups + 1) + 63) & ~(size_t)63; }
    // Where a batch of whole groups keeps its records, by record type: a projected batch has its n_groups read lengths
    // between the group offsets and the records.
    template <typename Rec>
    static size_t groups_records_at(uint64_t n_groups)
    {
        return std::is_same<Rec, oem_proj_record>::value ? records_at(2 * n_groups) : records_at(n_groups);
    }
    template <typename Rec>
    const Rec *records() const { return (const Rec *)((const char *)mem.p + groups_records_at<Rec>(n_groups)); }
    const uint64_t *read_len() const { return group_off() + n_groups + 1; } // (a projected batch)
    // the names form: offsets first (as group_off is), records at records_at(n_records), the bytes behind them
    const uint64_t *name_off() const { return (const uint64_t *)mem.p; }
    const oem_aln_record *named_records() const { return (const oem_aln_record *)((const char *)mem.p + records_at(n_records)); }
    static size_t names_at(uint64_t n_records) { return records_at(n_records) + ((sizeof(oem_aln_record) * n_records + 63) & ~(size_t)63); }
    const uint8_t *names() const { return (const uint8_t *)mem.p + names_at(n_records); }
    static size_t sec_at(uint64_t n_records, uint64_t name_bytes) { return names_at(n_records) + ((name_bytes + 63) & ~(size_t)63); }
    const uint8_t *secondary() const { return (const uint8_t *)mem.p + sec_at(n_records, name_bytes); }
};

// What a batch leaves on the device: r.row_ptr32 (n_rows + 1, from 0), r.tid, r.as_prob, with a model r.start / r.end /
// r.strand, r.n_kept (n_groups + 1) and r.dt.  A batch without groups leaves no arrays.
// A names session's piece holds the groups its batch CLOSED (oem_collate.h, the streamed rule), and besides the above:
// group_off (n_groups + 1 positions from 0 among the closed groups' records, n_records of them), the names of its rows
// as a dense blob (row_bytes) with row_off (n_rows + 1 offsets from 0), and the number of groups with n_kept == 1.
// A projected session's piece has `unsure`: the alignments whose as_prob slot still holds f (oem_filter_device.h).
struct Piece {
    FilterResult r;
    ProjDeferred unsure;
    uint64_t n_groups = 0;
    DevBuf<uint64_t> group_off, row_off;
    DevBuf<uint8_t> rows;
    uint64_t n_records = 0, row_bytes = 0, unique = 0;
};

// The head names of one batch's first closed groups, kept for the session's collation check: k names as a dense blob
// with k + 1 offsets from 0, and the heads' session-global input indices.
struct CheckChunk {
    DevBuf<uint8_t> blob;
    DevBuf<uint64_t> off, heads;
    uint64_t k = 0, bytes = 0;
};

// ---- the names session's kernels: one lane per word, nothing staged ------------------------------------------------------

// *equal = the name of record order[0] is the name of record `other`, byte for byte (one workgroup; names are short)
__global__ __launch_bounds__(kCT) void k_names_equal(const uint8_t *__restrict__ names, const uint64_t *__restrict__ name_off,
                                                     const uint32_t *__restrict__ order, uint64_t other, uint32_t *__restrict__ equal)
{
    const uint64_t i = order[0], a0 = name_off[i], la = name_off[i + 1] - a0, b0 = name_off[other], lb = name_off[other + 1] - b0;
    int diff = la != lb;
    if (!diff)
        for (uint64_t k = threadIdx.x; k < la; k += kCT) diff |= names[a0 + k] != names[b0 + k];
    diff = __syncthreads_or(diff);
    if (threadIdx.x == 0) *equal = diff ? 0u : 1u;
}

// The closed groups of a batch, the carry spliced in: group j's first position among the closed records (goff, nc + 1
// entries from 0) and the record that carries its name (head: an input index of the batch, or carry_rec for the group
// the carry opens).  c carry records come first; gb: the batch's own cut (positions among its survivors), order: the
// survivors' input indices.  first_is_carry: c > 0; shift 1: the carry closes as a group of its own, the batch's run b
// is group b + 1; shift 0: the batch's first run joins the carry (or there is no carry), run b is group b.
__global__ __launch_bounds__(kCT) void k_names_splice(uint64_t nc, uint64_t c, uint32_t shift, uint32_t first_is_carry,
                                                      const uint64_t *__restrict__ gb, const uint32_t *__restrict__ order, uint32_t carry_rec,
                                                      uint64_t *__restrict__ goff, uint32_t *__restrict__ head)
{
    const uint64_t j = (uint64_t)blockIdx.x * kCT + threadIdx.x;
    if (j > nc) return;
    if (j == nc) {
        goff[nc] = c + gb[nc - shift];
    } else if (first_is_carry && j == 0) {
        goff[0] = 0;
        head[0] = carry_rec;
    } else {
        const uint64_t p = gb[j - shift];
        goff[j] = c + p;
        head[j] = order[p];
    }
}

// out[j] = the session-global input index of head[j]
__global__ __launch_bounds__(kCT) void k_names_heads64(uint64_t k, const uint32_t *__restrict__ head, uint32_t carry_rec, uint64_t carry_head,
                                                       uint64_t rec_base, uint64_t *__restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * kCT + threadIdx.x;
    if (j < k) out[j] = head[j] == carry_rec ? carry_head : rec_base + head[j];
}

// out[row_idx[g]] = head[g] for the groups with n_kept > 0
__global__ __launch_bounds__(kCT) void k_names_row_heads(uint64_t nc, const uint32_t *__restrict__ n_kept, const uint64_t *__restrict__ row_idx,
                                                         const uint32_t *__restrict__ head, uint32_t *__restrict__ out)
{
    const uint64_t g = (uint64_t)blockIdx.x * kCT + threadIdx.x;
    if (g < nc && n_kept[g]) out[row_idx[g]] = head[g];
}

inline dim3 names_grid(uint64_t n) { return dim3((unsigned)std::max<uint64_t>((n + kCT - 1) / kCT, 1)); }

} // namespace
} // namespace oem

using namespace oem;

struct oem_records_stream {
    oem_records_stream_opts o;
    oem_filters f;
    std::vector<uint64_t> txp_len;
    std::vector<float> tab; // filter_prob_table of f.score_prob_denom
    bool host_only = false; // ... or there is none: the host loop takes every batch

    // The staging queue (oem_stage_queue.h): tickets, budget, arenas and the worker.  Its lock is the session's.
    StageQueue<Batch> q;
    std::mutex &mu = q.mu;
    std::vector<std::unique_ptr<Piece>> pieces; // by ticket
    uint64_t total_groups = 0, total_kept = 0;
    uint64_t before_finish = 0, host_batches = 0, names_unique = 0;
    bool finish_called = false;
    int sticky_rc = OEM_OK;
    std::string sticky_msg;

    explicit oem_records_stream(const oem_records_stream_opts &opts)
        : o(opts), q(opts.max_staged_records ? opts.max_staged_records : kDefaultMaxStaged, kPoolArenas,
                     [this](size_t bytes, StageMem *m) {
                         if (stage_host_alloc(o.device, bytes, m)) return true;
                         std::lock_guard<std::mutex> lk(mu);
                         set_sticky(OEM_ERR_OOM, "oem_records_stream_push: host allocation of the staging memory failed");
                         return false;
                     },
                     stage_host_free)
    {
    }
    void set_sticky(int rc, const char *msg) // (mu held)
    {
        if (sticky_rc != OEM_OK) return;
        sticky_rc = rc;
        sticky_msg = msg;
    }

    // -- the names session (oem_records_stream_set_names) --------------------------------------------------------------
    bool named = false;
    uint64_t sort_check_num = 0;
    // the carry: the open read's surviving records and its one name, on the device; its head and sizes on the host
    DevBuf<oem_aln_record> carry;
    DevBuf<uint8_t> carry_name;
    uint64_t carry_cap = 0, carry_n = 0, carry_head = 0, carry_len = 0;
    uint64_t n_unmapped = 0, n_parsed = 0;
    // the collation check: the head names of the first closed groups until sort_check_num are held or finish comes
    std::vector<std::unique_ptr<CheckChunk>> chk;
    uint64_t chk_held = 0;
    bool chk_done = false;
    // what finish leaves for oem_records_stream_names_copy
    bool names_ready = false;
    std::vector<uint64_t> out_group_off, out_row_off;
    std::vector<uint32_t> out_kept;
    std::vector<uint8_t> out_rows;

    // -- the sorting names session (oem_records_stream_set_sort): `named` too ------------------------------------------------
    bool sorting = false;
    SurvivorArena arena{1024, 4096, false, false}; // the survivors of all batches so far, in ticket order (the worker's alone)
    bool any_sec = false;            // a batch has brought flags
    uint64_t arena_peak = 0;         // (mu held) arena.peak as of the last batch
    std::vector<uint64_t> out_order; // what finish leaves for oem_records_stream_order_copy

    // -- the projected session (oem_records_stream_set_projected) --------------------------------------------------------
    bool projected = false;
    oem_proj_opts popts{10.f, OEM_PROJ_SIMILARITY};
    uint64_t host_finished = 0; // after finish: alignments whose expf the host supplied

    // the session's kind as the calls name it: 0 plain, 1 names, 2 projected, 3 sorting names (mu held)
    int kind() const { return sorting ? 3 : named ? 1 : projected ? 2 : 0; }

    template <typename Rec>
    int run_batch(const Batch &b, Piece *out, bool *host);
    int run_batch_names(const Batch &b, Piece *out, bool *host);
    int run_batch_sort(const Batch &b);
    int finish_sort(const char *who, const oem_store_opts *opts, oem_discard_table *out_discard, oem_parse_info *pi, oem_store **out);
    int upload_piece(oem_builder &hb, const std::vector<uint32_t> &kept, uint64_t n_groups, const char *who, Piece *out);
    int close_groups(const char *who, uint64_t rec_base, uint64_t n, const oem_aln_record *h_records,
                     const oem_aln_record *d_in, const uint32_t *d_order, uint64_t p_last, const uint64_t *d_gb, uint64_t ngb, bool joins,
                     const uint8_t *d_names, const uint64_t *d_name_off, Piece *out, bool *host);
    int carry_append(const char *who, uint64_t rec_base, const oem_aln_record *h_records, const oem_aln_record *d_in, const uint32_t *d_order,
                     uint64_t cnt);
    int run_check(const char *who);
    int names_close(const char *who);
    int host_piece(const oem_aln_record *records, const uint64_t *group_off, uint64_t n_groups, const char *who, Piece *out);
    void process(Batch &b, bool skip);
    int join(const char *who, FilterResult *out, uint64_t *n_groups);
    int finish_begin(const char *who, bool names_form);
};

// The host loop on one batch (a fresh builder: bases 0), and its arrays uploaded as the piece.
int oem_records_stream::host_piece(const oem_aln_record *records, const uint64_t *group_off, uint64_t n_groups, const char *who, Piece *out)
{
    oem_builder hb;
    hb.f = f;
    hb.txp_len = txp_len;
    std::vector<uint32_t> kept(n_groups + 1, 0);
    OEM_TRY(add_groups_host(&hb, records, group_off, n_groups, kept.data(), who));
    return upload_piece(hb, kept, n_groups, who, out);
}

// The arrays of a scratch builder that has taken one batch (kept: n_groups + 1 entries, the last one 0) as the piece.
int oem_records_stream::upload_piece(oem_builder &hb, const std::vector<uint32_t> &kept, uint64_t n_groups, const char *who, Piece *out)
{
    FilterResult &r = out->r;
    r.row_ptr32.reset(); // (a device pass that met a big score has left n_kept behind)
    r.n_kept.reset();
    const uint64_t nnz = hb.tid.size(), n_rows = hb.row_ptr.size() - 1;
    if (nnz >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: a resident store needs fewer than 2^32 alignments", who);
    std::vector<uint32_t> rp32(hb.row_ptr.begin(), hb.row_ptr.end());
    auto up = [&](auto *dbuf, const auto *src, uint64_t n) -> int {
        OEM_TRY(dev_alloc(&dbuf->p, n, nullptr));
        if (n) OEM_HIP(hipMemcpy(dbuf->p, src, sizeof(*src) * n, hipMemcpyHostToDevice));
        return OEM_OK;
    };
    OEM_TRY(up(&r.row_ptr32, rp32.data(), n_rows + 1));
    OEM_TRY(up(&r.n_kept, kept.data(), n_groups + 1));
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

// One batch of whole groups, for either record type: the one call's pass with base 0 straight from the arena, or --
// the one call's fallbacks -- the host loop into a scratch builder.  A projected batch leaves its unsure alignments in
// the piece's list (proj_device with `deferred`); the host loop's as_prob is final and its list is empty.
template <typename Rec>
int oem_records_stream::run_batch(const Batch &b, Piece *out, bool *host)
{
    constexpr bool kProj = std::is_same<Rec, oem_proj_record>::value;
    out->n_groups = b.n_groups;
    if (b.n_groups == 0) return OEM_OK;
    char who[64];
    snprintf(who, sizeof who, "oem_records_stream: ticket %llu", (unsigned long long)b.ticket);
    const Rec *records = b.records<Rec>();
    if (!host_only) {
        if constexpr (kProj) {
            OEM_TRY(proj_device(who, f, popts, txp_len.data(), o.n_txps, tab, records, b.group_off(), b.read_len(), b.n_groups, 0,
                                o.model >= 0, true, &out->r, &out->unsure, b.mem.pinned));
        } else {
            OEM_TRY(filter_device(who, f, txp_len.data(), o.n_txps, tab, records, b.group_off(), b.n_groups, 0, o.model >= 0, true,
                                  &out->r, nullptr, b.mem.pinned));
        }
        out->r.txp_len.reset(); // (the join uploads the lengths once)
        if (!out->r.host_rerun) return OEM_OK;
    }
    *host = true;
    if constexpr (kProj) {
        oem_builder hb;
        hb.f = f;
        hb.txp_len = txp_len;
        std::vector<uint32_t> kept(b.n_groups + 1, 0);
        OEM_TRY(add_projected_groups_host(&hb, records, b.group_off(), b.read_len(), b.n_groups, popts, kept.data(), who));
        return upload_piece(hb, kept, b.n_groups, who, out);
    } else {
        return host_piece(records, b.group_off(), b.n_groups, who, out);
    }
}

// ---- the names session's worker ("The names session") ---------------------------------------------

namespace oem {
namespace {

// Copy jobs for one k_stream_concat launch.
struct ConcatPlan {
    std::vector<ConcatJob> jobs;
    uint64_t n_blocks = 0;
    void add(const void *src, void *dst, uint64_t n, uint32_t elem, uint64_t add_)
    {
        if (n == 0) return;
        ConcatJob j{(const uint8_t *)src, (uint8_t *)dst, n * elem, n_blocks, add_, elem, 0};
        n_blocks += concat_blocks(j);
        jobs.push_back(j);
    }
    int run(const char *who, float *ms)
    {
        if (n_blocks > 0x7fffffffull) return fail(OEM_ERR_ARG, "%s: the join needs %llu workgroups", who, (unsigned long long)n_blocks);
        if (jobs.empty()) return OEM_OK;
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
        if (ms) OEM_HIP(hipEventElapsedTime(ms, ev[0].e, ev[1].e));
        return OEM_OK;
    }
};

int bad_ref(const char *who, uint64_t record, uint32_t ref_id)
{
    return fail(OEM_ERR_ARG, "%s: record %llu: ref_id %u is not below n_txps", who, (unsigned long long)record, ref_id);
}

} // namespace
} // namespace oem

// The survivors order[0 .. cnt) of the batch behind the carry's records, their ref_ids checked first: the carry holds
// only records the filter can take, so a ref_id error always names a record of the batch that is being worked on.
// The buffer doubles: a read that spans many batches is copied a constant number of times per record.
int oem_records_stream::carry_append(const char *who, uint64_t rec_base, const oem_aln_record *h_records, const oem_aln_record *d_in,
                                     const uint32_t *d_order, uint64_t cnt)
{
    if (!cnt) return OEM_OK;
    if (carry_n + cnt > 0xffffffffull)
        return fail(OEM_ERR_ARG, "%s: the read that starts at record %llu has more than 2^32 - 1 records", who, (unsigned long long)carry_head);
    uint64_t bad = kNoRecord;
    OEM_TRY(records_ref_check(cnt, d_order, d_in, o.n_txps, &bad));
    if (bad != kNoRecord) return bad_ref(who, rec_base + bad, h_records[bad].ref_id);
    if (carry_n + cnt > carry_cap) {
        const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(2 * carry_cap, carry_n + cnt), 64);
        DevBuf<oem_aln_record> grown;
        OEM_TRY(dev_alloc(&grown.p, cap, nullptr));
        if (carry_n) OEM_HIP(hipMemcpy(grown.p, carry.p, sizeof(oem_aln_record) * carry_n, hipMemcpyDeviceToDevice));
        std::swap(grown.p, carry.p);
        carry_cap = cap;
    }
    OEM_TRY(records_gather(cnt, d_order, d_in, carry.p + carry_n));
    carry_n += cnt;
    return OEM_OK;
}

// The session's collation check, once: the held head names joined into one blob (k_stream_concat) and the one call's
// check run over them.  The checked groups are the session's first ones, so the check's indices are group numbers.
int oem_records_stream::run_check(const char *who)
{
    chk_done = true;
    const uint64_t nchk = chk_held;
    uint64_t n_bytes = 0;
    for (const auto &c : chk) n_bytes += c->bytes;
    if (nchk > 1) {
        DevBuf<uint8_t> blob;
        DevBuf<uint64_t> off, heads;
        OEM_TRY(dev_alloc(&blob.p, n_bytes + 16, nullptr));
        OEM_TRY(dev_alloc(&off.p, nchk + 1, nullptr));
        OEM_TRY(dev_alloc(&heads.p, nchk, nullptr));
        OEM_HIP(hipMemset(blob.p + n_bytes, 0, 16));
        OEM_HIP(hipMemset(off.p, 0, sizeof(uint64_t)));
        ConcatPlan plan;
        uint64_t k0 = 0, b0 = 0;
        for (const auto &c : chk) {
            plan.add(c->blob.p, blob.p + b0, c->bytes, 1, 0);
            plan.add(c->off.p + 1, off.p + k0 + 1, c->k, 8, b0);
            plan.add(c->heads.p, heads.p + k0, c->k, 8, 0);
            k0 += c->k;
            b0 += c->bytes;
        }
        OEM_TRY(plan.run(who, nullptr));
        uint64_t found = ~0ull;
        OEM_TRY(parse_check_repeat(who, blob.p, off.p, n_bytes, nchk, &found));
        if (found != ~0ull) {
            const uint64_t g = found >> 32, earlier = found & 0xffffffffull;
            uint64_t rec_g = 0, rec_e = 0;
            OEM_HIP(hipMemcpy(&rec_g, heads.p + g, sizeof rec_g, hipMemcpyDeviceToHost));
            OEM_HIP(hipMemcpy(&rec_e, heads.p + earlier, sizeof rec_e, hipMemcpyDeviceToHost));
            chk.clear();
            return parse_not_collated(who, g, rec_g, rec_e);
        }
    }
    chk.clear();
    return OEM_OK;
}

// The groups a batch closes, filtered into its piece.  The batch: n records on the device (d_in) and in its arena
// (h_records), its survivors' input indices d_order, its own cut d_gb (ngb runs, the last one starting at survivor
// p_last), its names with the carry's name as record n + 1 (d_names / d_name_off).  Closed are the carry (with the
// batch's first run when `joins`) and every run but the last; finish closes the carry alone (n = 0, one empty run).
int oem_records_stream::close_groups(const char *who, uint64_t rec_base, uint64_t n, const oem_aln_record *h_records,
                                     const oem_aln_record *d_in, const uint32_t *d_order, uint64_t p_last, const uint64_t *d_gb, uint64_t ngb,
                                     bool joins, const uint8_t *d_names, const uint64_t *d_name_off, Piece *out, bool *host)
{
    const uint64_t c = carry_n;
    const uint32_t carry_rec = (uint32_t)(n + 1), shift = c > 0 && !joins ? 1u : 0u;
    const uint64_t nc = ngb - 1 + shift, tot = c + p_last;
    if (nc == 0) return OEM_OK;
    if (nc >= 0x7fffffffull) return fail(OEM_ERR_ARG, "%s: at most 2^31 - 2 reads per batch", who);
    DevBuf<oem_aln_record> d_comb; // the closed groups' records: the carry's, then the batch's survivors before its last run
    DevBuf<uint32_t> d_head;
    OEM_TRY(dev_alloc(&d_comb.p, tot, nullptr));
    OEM_TRY(dev_alloc(&d_head.p, nc, nullptr));
    OEM_TRY(dev_alloc(&out->group_off.p, nc + 1, nullptr));
    if (c) OEM_HIP(hipMemcpy(d_comb.p, carry.p, sizeof(oem_aln_record) * c, hipMemcpyDeviceToDevice));
    if (p_last) OEM_TRY(records_gather(p_last, d_order, d_in, d_comb.p + c));
    hipLaunchKernelGGL(k_names_splice, names_grid(nc + 1), dim3(kCT), 0, nullptr, nc, c, shift, c > 0 ? 1u : 0u, d_gb, d_order, carry_rec,
                       out->group_off.p, d_head.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipStreamSynchronize(nullptr));
    out->n_groups = nc;
    out->n_records = tot;

    // the collation check's share: the head names of the session's first sort_check_num groups
    if (sort_check_num && !chk_done && chk_held < sort_check_num) {
        std::unique_ptr<CheckChunk> ch(new CheckChunk());
        ch->k = std::min<uint64_t>(sort_check_num - chk_held, nc);
        OEM_TRY(gather_input_names(d_head.p, ch->k, d_names, d_name_off, &ch->off, &ch->blob, &ch->bytes));
        OEM_TRY(dev_alloc(&ch->heads.p, ch->k, nullptr));
        hipLaunchKernelGGL(k_names_heads64, names_grid(ch->k), dim3(kCT), 0, nullptr, ch->k, (const uint32_t *)d_head.p, carry_rec, carry_head,
                           rec_base, ch->heads.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipStreamSynchronize(nullptr));
        chk_held += ch->k;
        chk.push_back(std::move(ch));
        if (chk_held == sort_check_num) OEM_TRY(run_check(who));
    }

    // the filter over the closed groups as one cell; the host loop where the records session's would take the batch
    FilterResult &r = out->r;
    bool on_host = host_only;
    if (!on_host) {
        FilterCells fc;
        fc.n_cells = 1;
        DevBuf<unsigned long long> d_cell;
        const unsigned long long cell[2] = {0, nc};
        OEM_TRY(dev_alloc(&d_cell.p, 2, nullptr));
        OEM_HIP(hipMemcpy(d_cell.p, cell, sizeof cell, hipMemcpyHostToDevice));
        OEM_TRY(filter_device_resident(who, f, txp_len.data(), o.n_txps, tab, d_comb.p, (const unsigned long long *)out->group_off.p, nc,
                                       d_cell.p, o.model >= 0, &r, &fc));
        if (r.bad_ref_record != kNoRecord) { // (never one of the carry's: carry_append has checked those)
            if (r.bad_ref_record < c || !d_order) return fail(OEM_ERR_ARG, "%s: a carried record's ref_id is not below n_txps", who);
            uint32_t at = 0;
            OEM_HIP(hipMemcpy(&at, d_order + (r.bad_ref_record - c), sizeof at, hipMemcpyDeviceToHost));
            return bad_ref(who, rec_base + at, h_records[at].ref_id);
        }
        on_host = r.host_rerun;
    }
    if (on_host) { // the closed groups' records and offsets come down; the piece is uploaded
        *host = true;
        std::vector<oem_aln_record> recs(tot);
        std::vector<uint64_t> goff(nc + 1);
        if (tot) OEM_HIP(hipMemcpy(recs.data(), d_comb.p, sizeof(oem_aln_record) * tot, hipMemcpyDeviceToHost));
        OEM_HIP(hipMemcpy(goff.data(), out->group_off.p, sizeof(uint64_t) * (nc + 1), hipMemcpyDeviceToHost));
        for (uint64_t k = c; k < tot; ++k) {
            if (recs[k].ref_id < o.n_txps) continue;
            uint32_t at = 0;
            OEM_HIP(hipMemcpy(&at, d_order + (k - c), sizeof at, hipMemcpyDeviceToHost));
            return bad_ref(who, rec_base + at, recs[k].ref_id);
        }
        OEM_TRY(host_piece(recs.data(), goff.data(), nc, who, out));
    }
    d_comb.reset();
    r.txp_len.reset(); // (the join uploads the lengths once)

    // unique_alignments' share and the rows' names
    OEM_TRY(parse_count_unique(nc, r.n_kept.p, &out->unique));
    if (r.n_rows) {
        DevBuf<uint64_t> d_row_idx;
        DevBuf<uint32_t> d_row_head;
        OEM_TRY(dev_alloc(&d_row_idx.p, nc + 1, nullptr));
        OEM_TRY(dev_alloc(&d_row_head.p, r.n_rows, nullptr));
        OEM_TRY(parse_row_index(r.n_kept.p, nc + 1, d_row_idx.p)); // (n_kept has nc + 1 entries, the last one 0)
        hipLaunchKernelGGL(k_names_row_heads, names_grid(nc), dim3(kCT), 0, nullptr, nc, (const uint32_t *)r.n_kept.p,
                           (const uint64_t *)d_row_idx.p, (const uint32_t *)d_head.p, d_row_head.p);
        OEM_HIP(hipGetLastError());
        OEM_TRY(gather_input_names(d_row_head.p, r.n_rows, d_names, d_name_off, &out->row_off, &out->rows, &out->row_bytes));
    }
    return OEM_OK;
}

// One batch of a names session: upload from the arena, the survivors, their names checked, the adjacent cut, the carry
// spliced in, the closed groups filtered into the piece, the last run carried on.
int oem_records_stream::run_batch_names(const Batch &b, Piece *out, bool *host)
{
    const uint64_t n = b.n_records;
    if (n == 0) return OEM_OK;
    char who[64];
    snprintf(who, sizeof who, "oem_records_stream: ticket %llu", (unsigned long long)b.ticket);
    const uint64_t n_bytes = b.name_bytes, L = carry_n ? carry_len : 0;
    // the batch's names, 16 zero bytes (record n: never read), the carry's name as record n + 1, 16 zero bytes
    DevBuf<oem_aln_record> d_in;
    DevBuf<uint8_t> d_names;
    DevBuf<uint64_t> d_name_off;
    OEM_TRY(dev_alloc(&d_in.p, n, nullptr));
    OEM_HIP(hipMemcpyAsync(d_in.p, b.named_records(), sizeof(oem_aln_record) * n, hipMemcpyHostToDevice, nullptr));
    OEM_TRY(upload_blob_async(b.names(), n_bytes, b.name_off(), n, L + 16, 2, &d_names, &d_name_off));
    OEM_HIP(hipMemsetAsync(d_names.p + n_bytes + 16 + L, 0, 16, nullptr));
    if (L) OEM_HIP(hipMemcpyAsync(d_names.p + n_bytes + 16, carry_name.p, L, hipMemcpyDeviceToDevice, nullptr));
    const uint64_t tail[2] = {n_bytes + 16, n_bytes + 16 + L};
    OEM_HIP(hipMemcpy(d_name_off.p + n + 1, tail, sizeof tail, hipMemcpyHostToDevice));
    OEM_HIP(hipStreamSynchronize(nullptr));

    DevBuf<uint32_t> d_order;
    uint64_t m = 0;
    OEM_TRY(parse_survivors(d_in.p, n, true, &d_order, &m));
    n_unmapped += n - m;
    n_parsed += m;
    if (m == 0) return OEM_OK;
    const bool dense = m < n;
    CollateResident cr;
    {
        DevBuf<uint8_t> d_dense, d_dense_sec;
        DevBuf<uint64_t> d_dense_off;
        uint64_t dense_bytes = n_bytes, bad_record = kNoRecord;
        bool zero_byte = false;
        OEM_TRY(parse_survivor_names(d_names.p, n_bytes, d_name_off.p, n, dense ? d_order.p : nullptr, m, nullptr, &d_dense, &d_dense_off,
                                     &d_dense_sec, &dense_bytes, &bad_record, &zero_byte));
        if (bad_record != kNoRecord) return parse_bad_name(who, zero_byte, b.rec_base + bad_record);
        const uint64_t one_cell[2] = {0, m};
        CollateInput in;
        in.who = who;
        in.cell_rec_off = one_cell;
        in.mode = kCollateAdjacent;
        in.chunk_bytes = collate_chunk_bytes();
        in.d_names = dense ? d_dense.p : d_names.p;
        in.d_name_off = dense ? d_dense_off.p : d_name_off.p;
        in.d_n_bytes = dense_bytes;
        double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        OEM_TRY(collate_resident(in, 0, 1, 0, 0, 0, info, &cr));
    }
    cr.order.reset(); // (positions among the survivors: under ADJACENT the identity)
    const uint64_t ngb = cr.n_groups;
    uint64_t p_last = 0;
    OEM_HIP(hipMemcpy(&p_last, cr.group_off.p + (ngb - 1), sizeof p_last, hipMemcpyDeviceToHost));
    bool joins = false;
    if (carry_n) {
        DevBuf<uint32_t> d_eq;
        uint32_t eq = 0;
        OEM_TRY(dev_alloc(&d_eq.p, 1, nullptr));
        hipLaunchKernelGGL(k_names_equal, dim3(1), dim3(kCT), 0, nullptr, (const uint8_t *)d_names.p, (const uint64_t *)d_name_off.p,
                           (const uint32_t *)d_order.p, n + 1, d_eq.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpy(&eq, d_eq.p, sizeof eq, hipMemcpyDeviceToHost));
        joins = eq != 0;
    }
    if (ngb == 1 && joins) // the whole batch is more of the open read
        return carry_append(who, b.rec_base, b.named_records(), d_in.p, d_order.p, m);
    OEM_TRY(close_groups(who, b.rec_base, n, b.named_records(), d_in.p, d_order.p, p_last, cr.group_off.p, ngb, joins, d_names.p,
                         d_name_off.p, out, host));
    // the batch's last run is the new carry: its head's index comes down, its name stays on the device
    uint32_t last_head = 0;
    OEM_HIP(hipMemcpy(&last_head, d_order.p + p_last, sizeof last_head, hipMemcpyDeviceToHost));
    const uint64_t off0 = b.name_off()[last_head], len = b.name_off()[last_head + 1] - off0;
    carry_n = 0;
    carry_head = b.rec_base + last_head;
    carry_name.reset();
    OEM_TRY(dev_alloc(&carry_name.p, len, nullptr));
    OEM_HIP(hipMemcpy(carry_name.p, d_names.p + off0, len, hipMemcpyDeviceToDevice));
    carry_len = len;
    return carry_append(who, b.rec_base, b.named_records(), d_in.p, d_order.p + p_last, m - p_last);
}

// What a names session's finish does between the worker's end and the join: the carry closes as a last piece, and the
// collation check runs if fewer than sort_check_num groups were ever held.
int oem_records_stream::names_close(const char *who)
{
    if (!named) return OEM_OK;
    if (carry_n) {
        const uint64_t L = carry_len, off[3] = {0, 16, 16 + L}, gb[1] = {0};
        DevBuf<uint8_t> d_names;
        DevBuf<uint64_t> d_name_off, d_gb;
        OEM_TRY(dev_alloc(&d_names.p, 16 + L + 16, nullptr));
        OEM_TRY(dev_alloc(&d_name_off.p, 3, nullptr));
        OEM_TRY(dev_alloc(&d_gb.p, 1, nullptr));
        OEM_HIP(hipMemset(d_names.p, 0, 16 + L + 16));
        OEM_HIP(hipMemcpy(d_names.p + 16, carry_name.p, L, hipMemcpyDeviceToDevice));
        OEM_HIP(hipMemcpy(d_name_off.p, off, sizeof off, hipMemcpyHostToDevice));
        OEM_HIP(hipMemcpy(d_gb.p, gb, sizeof gb, hipMemcpyHostToDevice));
        std::unique_ptr<Piece> piece(new Piece());
        bool host = false;
        OEM_TRY(close_groups(who, q.total_records, 0, nullptr, nullptr, nullptr, 0, d_gb.p, 1, false, d_names.p, d_name_off.p,
                             piece.get(), &host));
        total_kept += piece->r.nnz;
        total_groups += piece->n_groups;
        if (host) ++host_batches;
        pieces.push_back(std::move(piece));
        carry_n = 0;
        carry.reset();
        carry_name.reset();
        carry_cap = 0;
    }
    if (sort_check_num && !chk_done) OEM_TRY(run_check(who));
    return OEM_OK;
}

// ---- the sorting names session's worker and finish ("The sorting names session") -------------------

// One batch of a sorting names session: upload from the staging arena, the survivors, their names checked and made
// dense, their ref_ids checked, and all of it appended to the device arena.  Nothing is cut or filtered here.
int oem_records_stream::run_batch_sort(const Batch &b)
{
    const uint64_t n = b.n_records;
    if (n == 0) return OEM_OK;
    char who[64];
    snprintf(who, sizeof who, "oem_records_stream: ticket %llu", (unsigned long long)b.ticket);
    const uint64_t n_bytes = b.name_bytes;
    DevBuf<oem_aln_record> d_in;
    DevBuf<uint8_t> d_names, d_sec;
    DevBuf<uint64_t> d_name_off;
    OEM_TRY(dev_alloc(&d_in.p, n, nullptr));
    OEM_HIP(hipMemcpyAsync(d_in.p, b.named_records(), sizeof(oem_aln_record) * n, hipMemcpyHostToDevice, nullptr));
    OEM_TRY(upload_blob_async(b.names(), n_bytes, b.name_off(), n, 0, 0, &d_names, &d_name_off));
    if (b.has_sec) OEM_TRY(upload_flags_async(b.secondary(), n, &d_sec));
    OEM_HIP(hipStreamSynchronize(nullptr));

    DevBuf<uint32_t> d_order;
    uint64_t m = 0;
    OEM_TRY(parse_survivors(d_in.p, n, true, &d_order, &m));
    n_unmapped += n - m;
    if (m == 0) return OEM_OK;
    if (arena.n + m > kCollateMaxBatch)
        return fail(OEM_ERR_ARG, "%s: more than 2^31 - 2 surviving records in the session: the names are collated as one batch", who);
    const bool dense = m < n;
    DevBuf<uint8_t> d_dense, d_dense_sec;
    DevBuf<uint64_t> d_dense_off;
    uint64_t dense_bytes = n_bytes, bad_record = kNoRecord;
    bool zero_byte = false;
    OEM_TRY(parse_survivor_names(d_names.p, n_bytes, d_name_off.p, n, dense ? d_order.p : nullptr, m, d_sec.p, &d_dense, &d_dense_off,
                                 &d_dense_sec, &dense_bytes, &bad_record, &zero_byte));
    if (bad_record != kNoRecord) return parse_bad_name(who, zero_byte, b.rec_base + bad_record);
    uint64_t bad = kNoRecord;
    OEM_TRY(records_ref_check(m, d_order.p, d_in.p, o.n_txps, &bad));
    if (bad != kNoRecord) return bad_ref(who, b.rec_base + bad, b.named_records()[bad].ref_id);

    const uint8_t *src_sec = !b.has_sec ? nullptr : dense ? d_dense_sec.p : d_sec.p;
    OEM_TRY(arena.append(m, d_order.p, d_in.p, n, b.rec_base, dense ? d_dense.p : d_names.p, dense ? d_dense_off.p : d_name_off.p, dense_bytes,
                         src_sec, nullptr, nullptr, nullptr, 0));
    any_sec |= b.has_sec;
    n_parsed += m;
    return OEM_OK;
}

// A sorting names session's finish, after the worker's end: the one call's tail on the arena.
int oem_records_stream::finish_sort(const char *who, const oem_store_opts *opts, oem_discard_table *out_discard, oem_parse_info *pi,
                                    oem_store **out)
{
    pi->n_unmapped = n_unmapped;
    pi->n_parsed = n_parsed;
    pieces.clear();
    const uint64_t m = arena.n;
    if (m == 0) { // nothing survives: the store of no groups, as the one call makes it
        const uint64_t no_groups[1] = {0};
        arena.release();
        out_group_off.assign(1, 0);
        out_row_off.assign(1, 0);
        return oem_store_create_records(&f, txp_len.data(), o.n_txps, nullptr, no_groups, 0, o.bin_width, o.model, o.growth_rate, o.device,
                                        opts, nullptr, out_discard, out);
    }
    double last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ParseTail t;
    t.who = who;
    t.filters = &f;
    t.txp_len = txp_len.data();
    t.n_txps = o.n_txps;
    t.tab = &tab;
    t.host_only = host_only;
    t.mode = kCollateSort;
    t.bin_width = o.bin_width;
    t.model = o.model;
    t.growth_rate = o.growth_rate;
    t.device = o.device;
    t.opts = opts;
    t.m = m;
    t.dense_bytes = arena.names.n_bytes;
    std::swap(t.d_in.p, arena.rec.p); // (the arena's padding is what the tail asks of an uploaded input)
    std::swap(t.d_names.p, arena.names.bytes.p);
    std::swap(t.d_name_off.p, arena.names.off.p);
    if (any_sec) std::swap(t.d_sec.p, arena.sec.p);
    t.d_global = arena.gidx.p; // (stays the arena's until the tail is over)
    t.want_rows = true;
    t.on_groups = [&](uint64_t ng) {
        out_order.resize(m);
        out_group_off.resize(ng + 1);
        out_kept.resize(ng);
        t.out_order64 = out_order.data();
        t.out_group_off = out_group_off.data();
        t.out_kept = out_kept.data();
    };
    t.on_rows = [&](uint64_t n_rows, uint64_t row_bytes) {
        out_row_off.resize(n_rows + 1);
        out_rows.resize(row_bytes);
        t.out_row_name_off = out_row_off.data();
        t.out_row_names = out_rows.data();
    };
    t.out_discard = out_discard;
    t.pi = pi;
    t.last = last;
    t.out = out;
    const int rc = parse_tail(t);
    arena.release();
    if (rc != OEM_OK) return rc;
    std::lock_guard<std::mutex> lk(mu);
    total_groups = pi->n_groups;
    if (last[3] != 0) ++host_batches;
    return OEM_OK;
}

// One batch on the queue's worker (oem_stage_queue.h), in ticket order.  skip: the session is cancelled or the batch was
// never staged; a stuck session skips too.  The queue takes the arena back and the records out of the budget behind this.
void oem_records_stream::process(Batch &b, bool skip)
{
    const bool dev_ok = hipSetDevice(o.device) == hipSuccess;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!dev_ok) set_sticky(OEM_ERR_HIP, "oem_records_stream: the device worker could not select its device");
        skip = skip || sticky_rc != OEM_OK;
        if (!skip && !finish_called) ++before_finish;
    }
    std::unique_ptr<Piece> piece;
    bool host = false;
    int rc = OEM_OK;
    std::string msg;
    if (!skip) {
        try {
            piece.reset(new Piece());
            rc = b.sorting     ? run_batch_sort(b)
                 : b.named     ? run_batch_names(b, piece.get(), &host)
                 : b.projected ? run_batch<oem_proj_record>(b, piece.get(), &host)
                               : run_batch<oem_aln_record>(b, piece.get(), &host);
        } catch (const std::bad_alloc &) {
            rc = fail(OEM_ERR_OOM, "oem_records_stream: host allocation failed in the device worker");
        } catch (const std::exception &e) {
            rc = fail(OEM_ERR_STATE, "oem_records_stream: %s", e.what());
        }
        if (rc != OEM_OK) {
            msg = last_error_text(); // (the message is thread-local)
            piece.reset();
            arena.release(); // (a sorting names session is stuck from here on: everything it held goes)
        }
    }
    std::lock_guard<std::mutex> lk(mu);
    arena_peak = arena.peak;
    if (rc != OEM_OK) {
        set_sticky(rc, msg.c_str());
    } else if (!skip) {
        total_kept += piece->r.nnz;
        if (b.named) total_groups += piece->n_groups;
        if (host) ++host_batches;
        if (total_kept >= (1ull << 32))
            set_sticky(OEM_ERR_ARG, "oem_records_stream: 2^32 or more alignments are kept; a resident store needs fewer");
        pieces[b.ticket] = std::move(piece);
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

    // a names session: group_off, the row names and their offsets are joined in the same launch
    DevBuf<uint64_t> d_goff, d_row_off;
    DevBuf<uint8_t> d_rows;
    uint64_t B = 0;
    if (named) {
        for (const auto &p : pieces) B += p->row_bytes;
        OEM_TRY(dev_alloc(&d_goff.p, G + 1, nullptr));
        OEM_TRY(dev_alloc(&d_row_off.p, R + 1, nullptr));
        OEM_TRY(dev_alloc(&d_rows.p, B, nullptr));
        OEM_HIP(hipMemset(d_goff.p, 0, sizeof(uint64_t)));
        OEM_HIP(hipMemset(d_row_off.p, 0, sizeof(uint64_t)));
    }

    // a projected session: the pieces' lists of unsure alignments are joined in the same launch, the indices made global
    DevBuf<uint64_t> d_uidx;
    DevBuf<float> d_uf;
    uint64_t U = 0, u0 = 0;
    for (const auto &p : pieces) U += p->unsure.n;
    if (U) {
        OEM_TRY(dev_alloc(&d_uidx.p, U, nullptr));
        OEM_TRY(dev_alloc(&d_uf.p, U, nullptr));
    }

    ConcatPlan plan;
    uint64_t *sum = &out->dt.discard_5p;
    uint64_t r0 = 0, a0 = 0, g0 = 0, p0 = 0, b0 = 0; // the piece's row, alignment, group, record and row-name byte base
    for (const auto &p : pieces) {
        if (p->unsure.n) {
            plan.add(p->unsure.idx.p, d_uidx.p + u0, p->unsure.n, 8, a0);
            plan.add(p->unsure.f.p, d_uf.p + u0, p->unsure.n, 4, 0);
            u0 += p->unsure.n;
        }
        const FilterResult &r = p->r;
        plan.add(r.n_kept.p, out->n_kept.p + g0, p->n_groups, 4, 0);
        plan.add(r.row_ptr32.p + 1, out->row_ptr32.p + r0 + 1, r.n_rows, 4, (uint32_t)a0);
        plan.add(r.tid.p, out->tid.p + a0, r.nnz, 4, 0);
        plan.add(r.as_prob.p, out->as_prob.p + a0, r.nnz, 4, 0);
        if (coords) {
            plan.add(r.start.p, out->start.p + a0, r.nnz, 4, 0);
            plan.add(r.end.p, out->end.p + a0, r.nnz, 4, 0);
            plan.add(r.strand.p, out->strand.p + a0, r.nnz, 1, 0);
        }
        if (named && p->n_groups) {
            plan.add(p->group_off.p + 1, d_goff.p + g0 + 1, p->n_groups, 8, p0);
            plan.add(p->row_off.p + 1, d_row_off.p + r0 + 1, r.n_rows, 8, b0);
            plan.add(p->rows.p, d_rows.p + b0, p->row_bytes, 1, 0);
        }
        for (int k = 0; k < kFilterCounters; ++k) sum[k] += (&r.dt.discard_5p)[k];
        names_unique += p->unique;
        r0 += r.n_rows;
        a0 += r.nnz;
        g0 += p->n_groups;
        p0 += p->n_records;
        b0 += p->row_bytes;
    }
    OEM_TRY(plan.run(who, &g_join_ms));
    // the deferred expf, once for the session: whatever reads the joined weights next sees them finished
    OEM_TRY(proj_finish_deferred(d_uidx.p, d_uf.p, U, out->as_prob.p));
    {
        std::lock_guard<std::mutex> lk(mu);
        host_finished = U;
    }
    if (named) { // the variable-length outputs stay with the session (oem_records_stream_names_copy)
        out_group_off.resize(G + 1);
        out_row_off.resize(R + 1);
        out_rows.resize(B);
        OEM_HIP(hipMemcpy(out_group_off.data(), d_goff.p, sizeof(uint64_t) * (G + 1), hipMemcpyDeviceToHost));
        OEM_HIP(hipMemcpy(out_row_off.data(), d_row_off.p, sizeof(uint64_t) * (R + 1), hipMemcpyDeviceToHost));
        if (B) OEM_HIP(hipMemcpy(out_rows.data(), d_rows.p, B, hipMemcpyDeviceToHost));
    }
    pieces.clear();
    *n_groups = G;
    return OEM_OK;
}

// What finish does before the join: the state checks, then the worker drains the queue and is joined.
int oem_records_stream::finish_begin(const char *who, bool names_form)
{
    {
        std::lock_guard<std::mutex> lk(mu);
        if (named && names_form && sticky_rc != OEM_OK) return fail(sticky_rc, "%s", sticky_msg.c_str()); // (sticky: every later call)
        if (named != names_form)
            return fail(OEM_ERR_STATE, names_form ? "%s: not a names session (oem_records_stream_set_names)"
                                                  : "%s: a names session is finished by oem_records_stream_finish_names", who);
        if (finish_called) return fail(OEM_ERR_STATE, "%s: the session is finished already", who);
        if (q.pushing) return fail(OEM_ERR_STATE, "%s: a push is in flight", who);
        finish_called = true;
    }
    q.close(); // (the worker runs what is staged)
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
    std::unique_ptr<oem_records_stream> s(new oem_records_stream(*opts));
    s->f = *filters;
    s->txp_len.assign(txp_len, txp_len + opts->n_txps);
    s->host_only = !filter_prob_table(filters->score_prob_denom, s->tab);
    oem_records_stream *raw = s.get();
    raw->q.start([raw](Batch &b, bool skip) { raw->process(b, skip); });
    *out = s.release();
    return OEM_OK;
    OEM_API_END("oem_records_stream_create")
}

namespace oem {
namespace {

// What the four pushes do once the batch's own checks have passed: the queue's push (oem_stage_queue.h) with the
// session's refusals as the status check, the batch's fields and its piece's slot as the initialiser, and fill(arena)
// to copy the caller's arrays.  kind: the session the push belongs to (oem_records_stream::kind()).  1: the batch of a
// names session (n_groups 0, name_bytes = name_off[n_records]); 2: of a projected session; 3: of a sorting names session
// (as 1, has_sec: with flags); a batch has a payload when `bytes` > 0.
template <typename Fill>
int stage_batch(oem_records_stream *s, const char *who, int kind, uint64_t n_groups, uint64_t n_records, uint64_t name_bytes, size_t bytes,
                Fill &&fill, uint64_t *out_ticket, bool has_sec = false)
{
    const bool named = kind == 1 || kind == 3;
    const int rc = s->q.push(
        n_records, bytes,
        [&](std::unique_lock<std::mutex> &) -> int {
            if (s->kind() != kind)
                return fail(OEM_ERR_STATE,
                            s->sorting  ? "%s: a sorting names session takes oem_records_stream_push_sort"
                            : kind == 3 ? "%s: not a sorting names session (oem_records_stream_set_sort)"
                            : kind == 1 ? "%s: not a names session (oem_records_stream_set_names)"
                            : kind == 2 ? "%s: not a projected session (oem_records_stream_set_projected)"
                            : s->named  ? "%s: a names session takes oem_records_stream_push_names"
                                        : "%s: a projected session takes oem_records_stream_push_projected",
                            who);
            if (named && s->sticky_rc != OEM_OK) return fail(s->sticky_rc, "%s", s->sticky_msg.c_str()); // (a names session: before all else)
            if (s->finish_called) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
            if (s->sticky_rc != OEM_OK) return fail(s->sticky_rc, "%s", s->sticky_msg.c_str());
            return OEM_OK;
        },
        [&](Batch &b) {
            s->pieces.reserve(s->pieces.size() + 2); // (whatever throws, throws here: + the carry's piece)
            s->pieces.emplace_back();
            b.n_groups = n_groups;
            b.named = named;
            b.projected = kind == 2;
            b.sorting = kind == 3;
            b.has_sec = has_sec;
            b.name_bytes = name_bytes;
            s->total_groups += n_groups;
        },
        fill, out_ticket);
    if (rc == kStageNoMemory) return fail(OEM_ERR_OOM, "%s: host allocation of the staging memory failed", who); // (sticky: the queue's alloc)
    return rc;
}

} // namespace
} // namespace oem

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
    return stage_batch(s, who, 0, n_groups, n_records, 0, n_groups ? bytes : 0, [&](char *mem) {
        std::memcpy(mem, group_off, sizeof(uint64_t) * (n_groups + 1));
        if (n_records) std::memcpy(mem + rec_at, records, sizeof(oem_aln_record) * n_records);
    }, out_ticket);
    OEM_API_END("oem_records_stream_push")
}

extern "C" int oem_records_stream_set_projected(oem_records_stream *s, const oem_proj_opts *popts)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_set_projected";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    const uint64_t no_groups[1] = {0};
    OEM_TRY(check_projected_batch(who, nullptr, no_groups, nullptr, 0, popts)); // (popts and its prob_source: the one call's check)
    std::vector<float> tab;
    const bool host_only = proj_host_only(s->f, *popts, &tab);
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->projected) return fail(OEM_ERR_STATE, "%s: the session is a projected session already", who);
    if (s->named) return fail(OEM_ERR_STATE, "%s: the session is a names session", who);
    if (s->finish_called) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
    if (s->q.next_ticket || s->q.pushing) return fail(OEM_ERR_STATE, "%s: a batch has been pushed already", who);
    s->projected = true;
    s->popts = *popts;
    s->host_only = host_only; // (the worker reads these two with its first batch, which no thread has pushed yet)
    s->tab.swap(tab);
    return OEM_OK;
    OEM_API_END("oem_records_stream_set_projected")
}

extern "C" int oem_records_stream_push_projected(oem_records_stream *s, const oem_proj_record *records, const uint64_t *group_off,
                                                 const uint64_t *read_len, uint64_t n_groups, uint64_t *out_ticket)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_push_projected";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    // the batch's own checks, on the calling thread, before the session is touched (the options are the session's)
    if (n_groups >= 0x7fffffffull) return fail(OEM_ERR_ARG, "%s: at most 2^31 - 2 groups per batch", who);
    const oem_proj_opts any{10.f, OEM_PROJ_SIMILARITY};
    OEM_TRY(check_projected_batch(who, records, group_off, read_len, n_groups, &any));
    const uint64_t n_records = group_off[n_groups];
    const size_t rec_at = Batch::groups_records_at<oem_proj_record>(n_groups), bytes = rec_at + sizeof(oem_proj_record) * n_records;
    return stage_batch(s, who, 2, n_groups, n_records, 0, n_groups ? bytes : 0, [&](char *mem) {
        std::memcpy(mem, group_off, sizeof(uint64_t) * (n_groups + 1));
        std::memcpy(mem + sizeof(uint64_t) * (n_groups + 1), read_len, sizeof(uint64_t) * n_groups);
        if (n_records) std::memcpy(mem + rec_at, records, sizeof(oem_proj_record) * n_records);
    }, out_ticket);
    OEM_API_END("oem_records_stream_push_projected")
}

extern "C" int oem_records_stream_set_names(oem_records_stream *s, uint64_t sort_check_num)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_set_names";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->named) return fail(OEM_ERR_STATE, "%s: the session is a names session already", who);
    if (s->projected) return fail(OEM_ERR_STATE, "%s: the session is a projected session", who);
    if (s->finish_called) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
    if (s->q.next_ticket || s->q.pushing) return fail(OEM_ERR_STATE, "%s: a batch has been pushed already", who);
    s->named = true;
    s->sort_check_num = sort_check_num;
    return OEM_OK;
    OEM_API_END("oem_records_stream_set_names")
}

extern "C" int oem_records_stream_push_names(oem_records_stream *s, const oem_aln_record *records, uint64_t n_records, const uint8_t *names,
                                             const uint64_t *name_off, uint64_t *out_ticket)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_push_names";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    // the batch's own checks, on the calling thread, before the session is touched
    if (!name_off) return fail(OEM_ERR_ARG, "%s: name_off is NULL", who);
    const uint64_t n = n_records, whole[2] = {0, n};
    if (n > kCollateMaxBatch) return fail(OEM_ERR_ARG, "%s: %llu records: at most 2^31 - 2 per batch", who, (unsigned long long)n);
    OEM_TRY(check_collate_input(who, names, name_off, n, whole, 1, kCollateAdjacent));
    if (n && !records) return fail(OEM_ERR_ARG, "%s: records is NULL", who);
    const uint64_t n_bytes = name_off[n];
    const size_t rec_at = Batch::records_at(n), names_at = Batch::names_at(n), bytes = names_at + n_bytes;
    return stage_batch(s, who, 1, 0, n, n_bytes, n ? bytes : 0, [&](char *mem) {
        std::memcpy(mem, name_off, sizeof(uint64_t) * (n + 1));
        std::memcpy(mem + rec_at, records, sizeof(oem_aln_record) * n);
        if (n_bytes) std::memcpy(mem + names_at, names, n_bytes);
    }, out_ticket);
    OEM_API_END("oem_records_stream_push_names")
}

extern "C" int oem_records_stream_set_sort(oem_records_stream *s)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_set_sort";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->sorting) return fail(OEM_ERR_STATE, "%s: the session is a sorting names session already", who);
    if (s->named) return fail(OEM_ERR_STATE, "%s: the session is a names session", who);
    if (s->projected) return fail(OEM_ERR_STATE, "%s: the session is a projected session", who);
    if (s->finish_called) return fail(OEM_ERR_STATE, "%s: the session is finished", who);
    if (s->q.next_ticket || s->q.pushing) return fail(OEM_ERR_STATE, "%s: a batch has been pushed already", who);
    s->named = true; // (finish_names, names_copy and the sticky rules are the names session's)
    s->sorting = true;
    s->sort_check_num = 0;
    return OEM_OK;
    OEM_API_END("oem_records_stream_set_sort")
}

extern "C" int oem_records_stream_push_sort(oem_records_stream *s, const oem_aln_record *records, uint64_t n_records, const uint8_t *names,
                                            const uint64_t *name_off, const uint8_t *secondary, uint64_t *out_ticket)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_push_sort";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    // the batch's own checks (oem_records_stream_push_names'), on the calling thread, before the session is touched
    if (!name_off) return fail(OEM_ERR_ARG, "%s: name_off is NULL", who);
    const uint64_t n = n_records, whole[2] = {0, n};
    if (n > kCollateMaxBatch) return fail(OEM_ERR_ARG, "%s: %llu records: at most 2^31 - 2 per batch", who, (unsigned long long)n);
    OEM_TRY(check_collate_input(who, names, name_off, n, whole, 1, kCollateSort));
    if (n && !records) return fail(OEM_ERR_ARG, "%s: records is NULL", who);
    const uint64_t n_bytes = name_off[n];
    const size_t rec_at = Batch::records_at(n), names_at = Batch::names_at(n), sec_at = Batch::sec_at(n, n_bytes);
    const size_t bytes = secondary ? sec_at + n : names_at + n_bytes;
    return stage_batch(s, who, 3, 0, n, n_bytes, n ? bytes : 0, [&](char *mem) {
        std::memcpy(mem, name_off, sizeof(uint64_t) * (n + 1));
        std::memcpy(mem + rec_at, records, sizeof(oem_aln_record) * n);
        if (n_bytes) std::memcpy(mem + names_at, names, n_bytes);
        if (secondary) std::memcpy(mem + sec_at, secondary, n);
    }, out_ticket, secondary != nullptr && n > 0);
    OEM_API_END("oem_records_stream_push_sort")
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
    OEM_TRY(s->finish_begin(who, false));
    FilterResult r;
    uint64_t n_groups = 0;
    OEM_TRY(s->join(who, &r, &n_groups));
    return filter_result_to_store(who, r, s->o.n_txps, n_groups, s->o.bin_width, s->o.model, s->o.growth_rate, s->o.device, opts,
                                  out_kept, out_discard, out);
    OEM_API_END("oem_records_stream_finish")
}

extern "C" int oem_records_stream_finish_names(oem_records_stream *s, const oem_store_opts *opts, oem_discard_table *out_discard,
                                               oem_parse_info *out_info, oem_store **out)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_finish_names";
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    OEM_TRY(check_store_from_records(who, &s->f, s->txp_len.data(), s->o.n_txps, s->o.bin_width, s->o.model, opts));
    OEM_TRY(s->finish_begin(who, true));
    oem_parse_info pi;
    std::memset(&pi, 0, sizeof pi);
    if (s->sorting) { // the one call's tail on the arena; the variable-length outputs stay with the session as below
        OEM_TRY(s->finish_sort(who, opts, out_discard, &pi, out));
        if (out_info) *out_info = pi;
        std::lock_guard<std::mutex> lk(s->mu);
        s->names_ready = true;
        return OEM_OK;
    }
    OEM_TRY(s->names_close(who));
    FilterResult r;
    uint64_t n_groups = 0;
    OEM_TRY(s->join(who, &r, &n_groups));
    pi.n_unmapped = s->n_unmapped;
    pi.n_parsed = s->n_parsed;
    pi.n_groups = n_groups;
    pi.n_reads = r.n_rows;
    pi.unique_alignments = s->names_unique;
    pi.n_checked = s->sort_check_num ? std::min<uint64_t>(s->sort_check_num, n_groups) : 0;
    s->out_kept.assign(n_groups + 1, 0);
    OEM_TRY(filter_result_to_store(who, r, s->o.n_txps, n_groups, s->o.bin_width, s->o.model, s->o.growth_rate, s->o.device, opts,
                                   s->out_kept.data(), out_discard, out));
    s->out_kept.resize(n_groups);
    if (out_info) *out_info = pi;
    std::lock_guard<std::mutex> lk(s->mu);
    s->names_ready = true;
    return OEM_OK;
    OEM_API_END("oem_records_stream_finish_names")
}

extern "C" int oem_records_stream_names_copy(const oem_records_stream *s, uint64_t *out_group_off, uint32_t *out_kept, uint8_t *out_row_names,
                                             uint64_t *out_row_name_off)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_names_copy";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    if ((out_row_names == nullptr) != (out_row_name_off == nullptr))
        return fail(OEM_ERR_ARG, "%s: out_row_names and out_row_name_off must both be NULL or both be given", who);
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->names_ready) return fail(OEM_ERR_STATE, "%s: no names session has been finished", who);
    if (out_group_off) std::memcpy(out_group_off, s->out_group_off.data(), sizeof(uint64_t) * s->out_group_off.size());
    if (out_kept && !s->out_kept.empty()) std::memcpy(out_kept, s->out_kept.data(), sizeof(uint32_t) * s->out_kept.size());
    if (out_row_names) {
        if (!s->out_rows.empty()) std::memcpy(out_row_names, s->out_rows.data(), s->out_rows.size());
        std::memcpy(out_row_name_off, s->out_row_off.data(), sizeof(uint64_t) * s->out_row_off.size());
    }
    return OEM_OK;
    OEM_API_END("oem_records_stream_names_copy")
}

extern "C" int oem_records_stream_order_copy(const oem_records_stream *s, uint64_t *out_order)
{
    OEM_API_BEGIN
    const char *who = "oem_records_stream_order_copy";
    if (!s) return fail(OEM_ERR_ARG, "%s: NULL session", who);
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->sorting) return fail(OEM_ERR_STATE, "%s: not a sorting names session (oem_records_stream_set_sort)", who);
    if (!s->names_ready) return fail(OEM_ERR_STATE, "%s: the session has not been finished", who);
    if (!out_order && !s->out_order.empty()) return fail(OEM_ERR_ARG, "%s: out_order is NULL", who);
    if (!s->out_order.empty()) std::memcpy(out_order, s->out_order.data(), sizeof(uint64_t) * s->out_order.size());
    return OEM_OK;
    OEM_API_END("oem_records_stream_order_copy")
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
    if (s->sorting) return fail(OEM_ERR_STATE, "%s: a sorting names session has no joined CSR", who);
    OEM_TRY(s->finish_begin(who, s->named));
    OEM_TRY(s->names_close(who)); // (a names session: the carry's piece and the check; the joined CSR is the same kind)
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
    case OEM_RECORDS_STREAM_INFO_BATCHES: *value = s->q.next_ticket; break;
    case OEM_RECORDS_STREAM_INFO_GROUPS: *value = s->total_groups; break;
    case OEM_RECORDS_STREAM_INFO_RECORDS: *value = s->q.total_records; break;
    case OEM_RECORDS_STREAM_INFO_BATCHES_BEFORE_FINISH: *value = s->before_finish; break;
    case OEM_RECORDS_STREAM_INFO_BLOCKED_US: *value = s->q.blocked_us; break;
    case OEM_RECORDS_STREAM_INFO_HOST_BATCHES: *value = s->host_batches; break;
    case OEM_RECORDS_STREAM_INFO_ROW_NAME_BYTES: *value = s->out_rows.size(); break;
    case OEM_RECORDS_STREAM_INFO_HOST_FINISHED: *value = s->host_finished; break;
    case OEM_RECORDS_STREAM_INFO_ARENA_BYTES: *value = s->arena_peak; break;
    default: return fail(OEM_ERR_ARG, "oem_records_stream_info: unknown key %u", key);
    }
    return OEM_OK;
}

extern "C" void oem_records_stream_destroy(oem_records_stream *s)
{
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        s->finish_called = true;
    }
    s->q.cancel(); // staged batches are dropped; the batch on the device runs to its end
    (void)hipSetDevice(s->o.device); // the pieces and the page-locked arenas are released on their device
    delete s;
}
