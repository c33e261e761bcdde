// oem_driver.h -- what the host-side drivers of the C ABI share (not part of the ABI): the store life cycle
// lives in oem_api.hip, the EM loop in oem_em_driver.hip, the bootstrap chains in oem_bootstrap.hip, the per-cell
// batches in oem_cells.hip and the HIP-event timing entry points in oem_timing.hip.
#pragma once

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "oem_internal.h"

// The host-side store builder (oem_builder.cpp); the batch entry points of oem_filter_device.hip append to it.
struct oem_builder {
    oem_filters f;
    std::vector<uint64_t> txp_len;
    std::vector<uint64_t> row_ptr{0};           // boundaries, starts [0] (oarfish_types.rs:645)
    std::vector<uint32_t> tid, start, end;
    std::vector<uint8_t> strand;
    std::vector<float> as_prob;
    oem_discard_table dt{};
};

// What oem_assignment_text, oem_assignment_text_lz4 (oem_assignment_text.hip), oem_count_matrix_text
// (oem_count_matrix_text.hip), oem_quant_text and oem_ambig_text (oem_quant_text.hip) return; read through oem_text_result_dims / _copy / _info.
struct oem_text_result {
    uint64_t n_bytes = 0;
    uint64_t n_lines = 0;
    uint64_t n_kept = 0;
    // oem_assignment_text_lz4: text is one LZ4 frame of content_bytes (prefix + body) in n_blocks blocks
    uint64_t content_bytes = 0, n_blocks = 0, raw_blocks = 0;
    std::unique_ptr<uint8_t[]> text;  // n_bytes
    std::vector<uint64_t> line_off;   // n_lines + 1
    std::vector<uint32_t> kept;       // n_lines
};

namespace oem {

const char *last_error_text(); // this thread's message (oem_last_error)

int comm_rank(const Comm *c);
int comm_size(const Comm *c);
bool comm_exchanges(const Comm *c);

// OEM_VERBOSE=1: wall-clock breakdown of store creation on stderr (upload / layout diagnostics)
struct StageTimer {
    bool on = getenv("OEM_VERBOSE") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char *what)
    {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[oem] %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

int ensure_device(int device);

template <typename T>
int dev_alloc(T **p, size_t n, uint64_t *acct)
{
    *p = nullptr;
    const size_t bytes = (n ? n : 1) * sizeof(T);
    OEM_HIP(hipMalloc((void **)p, bytes));
    if (acct) *acct += bytes;
    return OEM_OK;
}

// A device buffer that is freed with its scope (filled through dev_alloc(&b.p, ...) or hipMalloc).
template <typename T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { (void)hipFree(p); }
    void reset()
    {
        (void)hipFree(p);
        p = nullptr;
    }
};

// oem_api.hip: checks of the caller's arrays, store creation and destruction
int validate_csr(const uint64_t *row_ptr, const uint32_t *tid, uint64_t n_reads, uint64_t nnz, uint32_t n_txps);
uint64_t zero_nan_rows(const uint64_t *row_ptr, const double *cov, uint64_t n_reads, uint64_t nnz, std::vector<double> *fixed);

// Per-cell batches: cell c's transcripts are relabelled to [c * cell_txps, (c + 1) * cell_txps) -- on
// the device, after the upload, instead of in a second host copy of the transcript ids.
struct CellRelabel {
    const uint64_t *cell_row_off;
    uint32_t n_cells;
    uint32_t cell_txps;
    const unsigned long long *d_cell_row_off = nullptr; // the same offsets on the device already, or NULL
};
// A caller-order CSR already resident on the device (u32 row pointers, transcript ids, and either the f64 weights
// w = p * cov or, for an f32 store, the weights already rounded once to f32 in w32): a store created from it takes the
// buffers over (nulls them here) instead of uploading the caller's arrays.  Whatever is still held here is freed with
// it.
struct ResidentCsr {
    uint32_t *row_ptr = nullptr;
    uint32_t *tid = nullptr;
    double *w64 = nullptr;
    float *w32 = nullptr; // (set: an f32 store; w64 stays null)
    // A resident CSR without a host row_ptr (create_store_impl is given NULL): the host layout builder, which takes
    // the stores the device builder declines, asks for one here (NULL: allocation failed)
    const uint64_t *(*host_row_ptr)(void *) = nullptr;
    void *host_row_ptr_ctx = nullptr;
    // ... and, where the transcript ids have no host copy either (create_store_impl is given a NULL tid), for those
    const uint32_t *(*host_tid)(void *) = nullptr;
    ResidentCsr() = default;
    ResidentCsr(const ResidentCsr &) = delete;
    ResidentCsr &operator=(const ResidentCsr &) = delete;
    ~ResidentCsr()
    {
        (void)hipFree(row_ptr);
        (void)hipFree(tid);
        (void)hipFree(w64);
        (void)hipFree(w32);
    }
};
// With `resident`, tid / row_ptr are still the caller's host arrays in the same order (the host layout builder reads
// them) and as_prob / cov_prob are not read: the weights come from the resident buffers.  A store from a resident CSR
// takes its weights as given (weight_coding 2 is refused: the caller rounds them into w32 and asks for coding 1); a
// per-cell batch (relabel) from one keeps f64 weights and the device layout builder.
int create_store_impl(const uint64_t *row_ptr, const uint32_t *tid, const float *as_prob, const double *cov_prob,
                      uint64_t n_reads, uint64_t nnz, uint32_t n_txps, int device, const oem_store_opts *opts, oem_store *s,
                      const CellRelabel *relabel = nullptr, ResidentCsr *resident = nullptr);
void free_store(oem_store *s);
// The inverse: a per-cell batch the tiler declined hands the CSR back, with the caller's ids `tid` (host) again -- or,
// where they have no host copy (tid NULL), from their device copy d_tid.
int release_resident_csr(oem_store *s, ResidentCsr *resident, const uint32_t *tid, const uint32_t *d_tid = nullptr);
// u64 row pointers (host) -> u32 ones on the device, through a temporary u64 copy (no second host array)
int upload_row_ptr_u32(hipStream_t st, const uint64_t *row_ptr, uint64_t n, uint32_t *d_out);

// oem_coverage_cells.hip: the per-cell coverage model as the source of a cells EM's weights
// (oem_em_run_cells_coverage_sparse).  What the groups share is set up once per call; each group then computes its
// cells' coverage on the device from its own resident arrays and leaves the weights in a ResidentCsr
// (cells_coverage_group, oem_cells.h).
struct CellsCoverage {
    const uint32_t *aln_start = nullptr, *aln_end = nullptr; // host, caller order
    const uint64_t *txp_len = nullptr;                       // host, n_txps
    uint32_t n_txps = 0, bin_width = 0;
    int model = 1;
    double growth_rate = 2.0;
    double *out_cov_prob = nullptr; // host, nnz, or NULL
    // set up by cells_coverage_setup
    uint64_t *d_len = nullptr;
    uint32_t *d_nb = nullptr;
    uint32_t gerr = 0; // the annotation-wide checks: they fail every cell with alignments
    uint64_t all_bins = 0, max_nb = 0;
    CellsCoverage() = default;
    CellsCoverage(const CellsCoverage &) = delete;
    CellsCoverage &operator=(const CellsCoverage &) = delete;
    ~CellsCoverage()
    {
        (void)hipFree(d_len);
        (void)hipFree(d_nb);
    }
};
int cells_coverage_setup(CellsCoverage *cc);
// ... and the checks its entry points share, in this order: bin width, model, n_txps, nnz, n_reads
int check_cells_coverage_args(const char *who, uint32_t bin_width, int model, uint32_t n_txps, uint64_t nnz, uint64_t n_reads);
// oem_cells.hip: cell_row_off spans [0, n_reads] and does not decrease
int check_cell_row_off(const char *who, const uint64_t *cell_row_off, uint32_t n_cells, uint64_t n_reads);

// oem_em_driver.hip: one EM run with the loop state on the device
struct RunArgs {
    const double *init = nullptr; // host, n_txps, or NULL
    const uint32_t *d_row_w = nullptr; // device multiplicities or NULL
    uint64_t row_begin = 0, row_end = 0;
    uint64_t total_reads = 0; // em.rs:154 total_weight
    uint32_t max_iter = 1000;
    double conv_thresh = 1e-3;
    uint32_t min_iter_gate = 50;
    int64_t history_run = -1; // row of the store's RunHistory this run records into (history_begin); -1: no record
};
// OEM_OPT_RUN_HISTORY (oem_em_driver.hip).  history_begin opens the record of an oem_em_run / oem_bootstrap call
// (n_runs rows of min(K, max_iter) entries; with the option off it only drops the previous call's), history_end marks it
// readable.  ensure_history_buf (re)allocates a device record of n doubles; history_cap is this call's row length.
uint32_t history_cap(const oem_store *s, uint32_t max_iter);
int history_begin(oem_store *s, uint32_t n_runs, uint32_t max_iter);
void history_end(oem_store *s);
int ensure_history_buf(oem_store *s, double **buf, uint32_t *have, size_t n);
// the run on s->d_state: its record's address into the (freshly cleared) state words; cap = 0: nothing to do
int history_arm(oem_store *s, uint32_t cap);
// What a finished loop state (EmState, BatchState) tells the caller; extra_passes: the final pass of em.rs:245-252 where
// the state has not counted it.
template <typename State>
oem_run_info run_info_from(const State &h, uint32_t extra_passes)
{
    oem_run_info info;
    info.niter = h.niter;
    info.n_passes = h.n_passes + extra_passes;
    info.converged = h.converged;
    info.reserved = 0;
    info.rel_diff = h.last_rel;
    return info;
}
// The loop state of a run on s->d_state cleared (device and host copy) and its record armed; and the start of a classic
// loop around it: theta filled with `avg` (em.rs:165) or left as uploaded (init_abundances), the counts cleared.
int reset_loop_state(oem_store *s, uint32_t hist_cap);
int begin_classic_loop(oem_store *s, const EmParams &p, double avg, bool fill);
bool use_tiled(const oem_store *s, const RunArgs &a);
int enqueue_pass(oem_store *s, const RunArgs &a, const EmState *state);
int prepare_row_w(oem_store *s, const RunArgs &a);
int enqueue_iteration(oem_store *s, const RunArgs &a, const EmParams &p);
int run_em_device(oem_store *s, const RunArgs &a, oem_run_info *info);
bool deferred_reldiff_ok(const oem_store *s, const RunArgs &a);
int ensure_deferred(oem_store *s);
int enqueue_deferred_pass(oem_store *s, const RunArgs &a, const EmParams &p, double *const bufs[3], uint64_t i);
int copy_counts_out(oem_store *s, double *out);
int ensure_row_w(oem_store *s);

// A chunk of the loop as a hipGraph -- an experiment that stays reachable (OEM_GRAPH=1 in the test-only
// library), not the product path: replaying 16 iterations from an instantiated graph instead of launching
// their kernels one by one changes nothing measurable on MI355X (10 M reads: 0.2240 vs 0.2239 ms per
// iteration; 1 M reads: 38.1 vs 38.1-38.8 us, profiles/r03_notes.md) -- dependent launches on one stream
// already follow each other within ~1 us, and the host is far ahead of the device.  Nothing in an
// iteration carries a per-launch value (loop state, stopping rule and the peer-to-peer epoch live on the
// device), so one captured chunk serves a whole run.
constexpr uint32_t kGraphIters = 16;

struct ChunkGraph {
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    ChunkGraph() = default;
    ChunkGraph(const ChunkGraph &) = delete;
    ChunkGraph &operator=(const ChunkGraph &) = delete;
    ~ChunkGraph()
    {
        if (ge) hipGraphExecDestroy(ge);
        if (g) hipGraphDestroy(g);
    }
    bool ready() const { return ge != nullptr; }
};

// Captures `body` (kernel launches on `st` only) n times.  Returns OEM_OK with !out->ready() when the
// runtime declines (the caller then launches directly); an error only when `body` itself fails.
template <typename F>
int capture_chunk(hipStream_t st, uint32_t n, F &&body, ChunkGraph *out)
{
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return OEM_OK;
    }
    int rc = OEM_OK;
    for (uint32_t k = 0; k < n && rc == OEM_OK; ++k) rc = body();
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    if (rc != OEM_OK || e != hipSuccess || !g) {
        if (g) hipGraphDestroy(g);
        (void)hipGetLastError();
        return rc;
    }
    hipGraphExec_t ge = nullptr;
    if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess || !ge) {
        hipGraphDestroy(g);
        (void)hipGetLastError();
        return OEM_OK;
    }
    out->g = g;
    out->ge = ge;
    return OEM_OK;
}

// RCCL calls are not captured (a row shard that exchanges through RCCL launches directly); the
// peer-to-peer exchange is plain kernels.
inline bool graph_ok(const oem_store *s, size_t exchange_count = 0)
{
    return knob("OEM_GRAPH", 0) != 0 &&
           !comm_exchange_is_unconditional(s->comm, exchange_count ? exchange_count : s->csr.n_txps);
}

// oem_bootstrap.hip
int ensure_batch(oem_store *s, int chain);
bool can_batch(const oem_store *s);
int agree_any(oem_store *s, bool *flag);

// oem_cells.hip: timing of the last oem_em_run_cells call of this thread
void cells_last_timing(double *loop_ms, uint64_t *batched_passes);
// ... and its groups: [c0, c1) and 1 when the group ran batched, 0 when cell by cell (oem_debug_cells_last_paths)
struct CellsGroupPath {
    uint32_t c0, c1, batched;
    LaunchRecord launch; // a batched group: its store's record when the loop had ended (oem_debug_last_launch)
};
const std::vector<CellsGroupPath> &cells_last_paths();

// oem_assignment_text.hip: kernel time of this thread's last oem_assignment_text under OEM_TEXT_TIMING=1 (test-only
// library), from HIP events: ms of the measure kernel, the scan and the emit kernels (all chunks)
void text_last_timing(float *ms3);
// ... and of this thread's last oem_assignment_text_lz4: ms of k_lz4_blocks and of scan + k_lz4_gather (all chunks)
void text_lz4_last_timing(float *ms2);
// oem_count_matrix_text.hip: the same three of this thread's last oem_count_matrix_text under OEM_MTX_TIMING=1
void mtx_last_timing(float *ms3);
// oem_gene_counts.hip: this thread's last oem_cells_gene_counts: ms of the uploads with the key kernels behind them and
// of the read-back by the host clock (both are synchronous), under OEM_GENE_TIMING=1 (test-only library) ms of the sort
// and of the kernels and the scan behind it from HIP events, then the device bytes it held and its batches
void gene_counts_last_call(double *out6);
// oem_quant_text.hip: this thread's last oem_quant_text / oem_ambig_text: its chunks, the workgroup tiles that went
// through the LDS stage and those written directly, then ms of measure, scan and emit under OEM_QUANT_TIMING=1
void quant_last_call(double *out6);
// oem_collate_device.hip: this thread's last oem_collate_names: the key rounds it ran (the most of any batch), its upload
// chunks, its batches; under OEM_COLLATE_TIMING=1 ms of the name uploads and of the kernels behind each chunk (HIP events,
// summed over the chunks), of the rounds and the cut after the upload (HIP events), of the copies into pinned staging
// (host clock); the rounds that had to sort
void collate_last_call(double *out8);

// oem_lz4.hip: the device buffers the compression of one chunk owns; reused by the chunks that follow it on its stream
struct Lz4Chunk {
    uint8_t *slots = nullptr; // one bound-strided slot per block: its compressed payload
    uint64_t slots_cap = 0;
    uint32_t *sizes = nullptr, *sums = nullptr; // per block: bytes of the payload as stored, XXH32 of it
    uint64_t *offs = nullptr;                   // per block: its offset in `frame`; offs[n_blocks] = the frame's bytes
    uint64_t blocks_cap = 0;
    uint8_t *tmp = nullptr; // the scan's
    uint64_t tmp_cap = 0;
    uint8_t *frame = nullptr; // the chunk's blocks as the frame holds them: size word, payload, checksum each
    uint64_t frame_cap = 0;
    unsigned long long *d_raw = nullptr;
    uint64_t *h_info = nullptr; // pinned: [0] bytes of `frame`, [1] raw blocks, once the stream has passed the enqueue
    uint64_t n_blocks = 0;
    Lz4Chunk() = default;
    Lz4Chunk(const Lz4Chunk &) = delete;
    Lz4Chunk &operator=(const Lz4Chunk &) = delete;
    ~Lz4Chunk(); // the stream is idle
};
// the block length: 64 KiB (the test-only library: OEM_LZ4_BLOCK_BYTES, at most that)
uint32_t lz4_block_bytes();
uint64_t lz4_blocks_of(uint64_t n, uint32_t block_bytes);
// Enqueues blocks / scan / gather of the n device bytes at d_in on `st`, and the copy of the result's length to
// c.h_info.  d_in stays untouched until the stream has passed (raw blocks are gathered from it).  The events, where
// given, are recorded after k_lz4_blocks and after k_lz4_gather.
int lz4_chunk_enqueue(Lz4Chunk &c, const uint8_t *d_in, uint64_t n, uint32_t block_bytes, hipStream_t st,
                      hipEvent_t ev_blocks = nullptr, hipEvent_t ev_gather = nullptr);
// One complete frame (descriptor, blocks, EndMark) of n host bytes, through the same three steps; synchronises `st`.
int lz4_frame_from_host(const uint8_t *data, uint64_t n, hipStream_t st, std::unique_ptr<uint8_t[]> *out, uint64_t *out_len,
                        uint64_t *n_blocks, uint64_t *raw_blocks);

// oem_coverage_device.hip: the bulk coverage model on arrays already on the device (u32 row pointers, ids, coordinates,
// transcript lengths): the column into d_out and, with d_p, the store's weights w = (double)p * cov into d_w64 or,
// rounded once to f32, into d_w32 (exactly one of the two is set).
int coverage_resident(const uint32_t *d_row_ptr, const uint32_t *d_tid, const uint32_t *d_start, const uint32_t *d_end,
                      const uint64_t *d_txp_len, uint64_t n_reads, uint64_t nnz, uint32_t n_txps, uint32_t bin_width,
                      int model, double growth_rate, double *d_out, const float *d_p, double *d_w64, float *d_w32);

// oem_builder.cpp: what a batch call needs of the builder.  A mark taken before a batch restores the builder when the
// batch fails (builder_rollback), which is what makes the batch calls atomic.
struct BuilderMark {
    size_t n_row_ptr, nnz;
    oem_discard_table dt;
};
BuilderMark builder_mark(const oem_builder *b);
void builder_rollback(oem_builder *b, const BuilderMark &m);
int check_group_off(const char *who, const void *records, const uint64_t *group_off, uint64_t n_groups);
int add_groups_host(oem_builder *b, const oem_aln_record *records, const uint64_t *group_off, uint64_t n_groups,
                    uint32_t *out_kept, const char *who);
// oem_builder_projected.cpp: the host loop of a projected batch (atomic, as add_groups_host) and the checks every
// projected batch call makes first
int add_projected_groups_host(oem_builder *b, const oem_proj_record *records, const uint64_t *group_off,
                              const uint64_t *read_len, uint64_t n_groups, const oem_proj_opts &popts, uint32_t *out_kept,
                              const char *who);
int check_projected_batch(const char *who, const oem_proj_record *records, const uint64_t *group_off,
                          const uint64_t *read_len, uint64_t n_groups, const oem_proj_opts *popts);

// oem_filter_device.hip: times of this thread's last device batch call under OEM_FILTER_TIMING=1 (test-only library; all
// zero when the call never reached the device pass): from HIP events, ms of the record uploads (sum over the chunks), of
// k_filter_measure (sum), of the two scans, of k_filter_emit, and the fraction of the measure kernels' time during which
// a record copy was in flight; from the host clock, ms the calling thread spent copying the records into pinned staging
void filter_last_timing(float *ms6);
void filter_timing_reset();
// oem_filter_projected_device.hip: this thread's last projected device batch call (test-only library): ms of
// k_proj_measure (summed over the chunks), of k_proj_emit, and of finishing the unsure alignments on the host (select,
// copy down, libm expf, copy up, scatter) -- the first two from HIP events under OEM_FILTER_TIMING=1, the third from the
// host clock -- then the number of alignments the host finished and the number emitted.  All zero when the call never
// reached the device pass; out[1] is zero when the host loop took the batch after the measure pass.
void proj_last_pass(double *out5);

} // namespace oem
