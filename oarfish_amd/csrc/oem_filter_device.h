// oem_filter_device.h -- what the two device filters share (oem_filter_device.hip: AlignmentFilters::filter,
// oem_filter_projected_device.hip: filter_projected): the chunked upload of the records with the measure kernel behind
// each chunk, the scans from n_kept to offsets, the result of a pass and what is made of it (the builder's arrays or a
// resident store).  The record type, the two kernels and how as_prob comes about are each file's own.
#pragma once

#include <cstring>
#include <vector>

#include "oem_driver.h"
#include "oem_filter.h"

namespace oem {

constexpr int kFT = 256;
constexpr uint64_t kFilterChunkGroups = 1ull << 18; // groups per upload chunk (the test-only library: OEM_FILTER_CHUNK_GROUPS)
constexpr unsigned long long kNoRecord = ~0ull;

// what a measure pass leaves besides its per-group arrays
struct FilterTotals {
    unsigned long long counts[kFilterCounters]; // oem_discard_table's order
    unsigned long long bad_record;              // the first record with an argument error (kNoRecord: none)
    uint32_t flags;
    uint32_t pad;
};

struct Stream {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
};
struct Event {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
};
struct Pinned {
    void *p = nullptr;
    ~Pinned() { if (p) (void)hipHostFree(p); }
};

// What a device filter pass returns: the new reads' CSR on the device.  row_ptr has n_rows + 1 entries, the first one
// `base`; exactly one of row_ptr64 / row_ptr32 is filled.
struct FilterResult {
    uint64_t n_rows = 0, nnz = 0;
    DevBuf<uint64_t> row_ptr64;
    DevBuf<uint32_t> row_ptr32, tid, start, end, n_kept;
    DevBuf<float> as_prob;
    DevBuf<uint8_t> strand;
    DevBuf<uint64_t> txp_len; // the transcript lengths, kept for the coverage model
    oem_discard_table dt{};
    bool host_rerun = false;  // a score beyond +-2^24: nothing above is filled, the host loop takes the batch
    unsigned long long bad_ref_record = kNoRecord; // the resident form only: the first record whose ref_id is not below n_txps
};

// The per-cell form of a pass (oem_cells_records.hip): the batch's groups belong to n_cells consecutive cells, cell c
// owning groups [cell_group_off[c], cell_group_off[c + 1]) of the batch.  The pass then counts the discards per cell
// (k_filter_measure's per-cell form) and samples the two scans at the cells' first groups (k_filter_cell_offsets), so
// that the result is a group of the per-cell driver: d_cell_row_off is the device cell_row_off a CellsGroup takes.
struct FilterCells {
    const uint64_t *cell_group_off = nullptr; // host, n_cells + 1, from 0 to the batch's n_groups
    uint32_t n_cells = 0;
    uint64_t first_cell = 0, first_record = 0; // the batch's place in the call or session, for messages
    DevBuf<unsigned long long> d_cell_row_off, d_cell_aln_off;        // n_cells + 1 each
    std::vector<uint64_t> cell_row_off, cell_aln_off;                 // ... and on the host
    std::vector<oem_discard_table> tables;                            // n_cells
};

inline long filter_chunk_groups()
{
    const long ck = knob("OEM_FILTER_CHUNK_GROUPS", (long)kFilterChunkGroups);
    return ck > 0 ? ck : (long)kFilterChunkGroups;
}

// The records in chunks cut at group boundaries, from two pinned staging buffers, alternating between two streams:
// chunk k's measure kernel -- launch(stream, g0, g1) enqueues it -- runs while chunk k + 1 is copied.  The caller's array
// is pageable, so every chunk is first copied into its staging buffer by the calling thread.  Returns once both lanes are
// idle.  ms (6 floats, or NULL for no timing): [0] the uploads and [1] the measure kernels from HIP events, summed over
// the chunks, [4] the fraction of the measure kernels' time during which a record copy was in flight, [5] += the staging
// copies by the host clock.
// pinned_src: the caller's array is page-locked already (the records session's staging): the chunks are copied from it
// directly, there are no staging buffers and no staging copies.
template <typename Rec, typename Launch>
int filter_upload_measure(const Rec *records, Rec *d_recs, const uint64_t *group_off, uint64_t n_groups, uint64_t chunk,
                          float *ms, Launch &&launch, bool pinned_src = false)
{
    const bool timing = ms != nullptr;
    uint64_t max_chunk_records = 0;
    for (uint64_t g0 = 0; g0 < n_groups; g0 += chunk) {
        const uint64_t g1 = g0 + chunk < n_groups ? g0 + chunk : n_groups;
        if (group_off[g1] - group_off[g0] > max_chunk_records) max_chunk_records = group_off[g1] - group_off[g0];
    }
    Stream lane[2];
    Pinned stage[2];
    Event copied[2]; // the lane's last copy has left its staging buffer
    const uint64_t n_chunks = (n_groups + chunk - 1) / chunk;
    for (int l = 0; l < 2 && (uint64_t)l < n_chunks; ++l) {
        OEM_HIP(hipStreamCreateWithFlags(&lane[l].s, hipStreamNonBlocking));
        if (!pinned_src)
            OEM_HIP(hipHostMalloc(&stage[l].p, (max_chunk_records ? max_chunk_records : 1) * sizeof(Rec), hipHostMallocDefault));
        OEM_HIP(hipEventCreateWithFlags(&copied[l].e, hipEventDisableTiming));
    }
    struct ChunkEvents { hipEvent_t c0 = nullptr, c1 = nullptr, m1 = nullptr; };
    std::vector<ChunkEvents> cev(timing ? n_chunks : 0);
    struct EvGuard {
        std::vector<ChunkEvents> &v;
        ~EvGuard() { for (auto &c : v) { if (c.c0) (void)hipEventDestroy(c.c0); if (c.c1) (void)hipEventDestroy(c.c1); if (c.m1) (void)hipEventDestroy(c.m1); } }
    } ev_guard{cev};
    for (auto &c : cev) {
        OEM_HIP(hipEventCreate(&c.c0));
        OEM_HIP(hipEventCreate(&c.c1));
        OEM_HIP(hipEventCreate(&c.m1));
    }
    uint64_t ci = 0;
    for (uint64_t g0 = 0; g0 < n_groups; g0 += chunk, ++ci) {
        const int l = (int)(ci & 1);
        const uint64_t g1 = g0 + chunk < n_groups ? g0 + chunk : n_groups;
        const uint64_t r0 = group_off[g0], nr = group_off[g1] - r0;
        const Rec *src = records + r0;
        if (!pinned_src) {
            if (ci >= 2) OEM_HIP(hipEventSynchronize(copied[l].e));
            const auto t_stage = std::chrono::steady_clock::now();
            if (nr) std::memcpy(stage[l].p, records + r0, nr * sizeof(Rec));
            if (timing) ms[5] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_stage).count();
            src = (const Rec *)stage[l].p;
        }
        if (timing) OEM_HIP(hipEventRecord(cev[ci].c0, lane[l].s));
        if (nr) OEM_HIP(hipMemcpyAsync(d_recs + r0, src, nr * sizeof(Rec), hipMemcpyHostToDevice, lane[l].s));
        OEM_HIP(hipEventRecord(copied[l].e, lane[l].s));
        if (timing) OEM_HIP(hipEventRecord(cev[ci].c1, lane[l].s));
        launch(lane[l].s, g0, g1);
        OEM_HIP(hipGetLastError());
        if (timing) OEM_HIP(hipEventRecord(cev[ci].m1, lane[l].s));
    }
    for (int l = 0; l < 2; ++l)
        if (lane[l].s) OEM_HIP(hipStreamSynchronize(lane[l].s));
    if (timing && n_chunks) { // intervals relative to the first chunk's copy start; overlap of each measure with the copies
        std::vector<float> c0(n_chunks), c1(n_chunks), m1(n_chunks);
        for (uint64_t i = 0; i < n_chunks; ++i) {
            OEM_HIP(hipEventElapsedTime(&c0[i], cev[0].c0, cev[i].c0));
            OEM_HIP(hipEventElapsedTime(&c1[i], cev[0].c0, cev[i].c1));
            OEM_HIP(hipEventElapsedTime(&m1[i], cev[0].c0, cev[i].m1));
        }
        float up = 0.f, msr = 0.f, ov = 0.f;
        for (uint64_t i = 0; i < n_chunks; ++i) {
            up += c1[i] - c0[i];
            msr += m1[i] - c1[i];
            for (uint64_t j = 0; j < n_chunks; ++j) { // (copies of the other lane only: a lane's own work is serial)
                if (((i ^ j) & 1) == 0) continue;
                const float a = c1[i] > c0[j] ? c1[i] : c0[j], b = m1[i] < c1[j] ? m1[i] : c1[j];
                if (b > a) ov += b - a;
            }
        }
        ms[0] = up;
        ms[1] = msr;
        ms[4] = msr > 0.f ? ov / msr : 0.f;
    }
    return OEM_OK;
}

// oem_filter_device.hip --------------------------------------------------------------------------------------------------
// Measure, scans and emit of one batch on the current device: the body of oem_builder_add_groups_device and
// oem_store_create_records.  tab: filter_prob_table of F.score_prob_denom.  want_coords: start / end / strand too.
// narrow: u32 row pointers (the total is checked against 2^32 first).  An argument error found on the device (ref_id) is
// reported here.  cells (or NULL): the per-cell form -- its device and host offsets and its tables are filled, out->dt
// is their sum, and a ref_id error names the cell too.  pinned_src: as filter_upload_measure.
int filter_device(const char *who, const oem_filters &F, const uint64_t *txp_len, uint32_t n_txps, const std::vector<float> &tab,
                  const oem_aln_record *records, const uint64_t *group_off, uint64_t n_groups, uint64_t base, bool want_coords,
                  bool narrow, FilterResult *out, FilterCells *cells = nullptr, bool pinned_src = false);
// The resident form of the per-cell pass (oem_em_run_cells_records_names_sparse): the batch's records, its group_off
// (n_groups + 1, from 0) and its cells' cell_group_off (cells->n_cells + 1) are on the device already, so there are no
// upload lanes: one k_filter_measure launch over [0, n_groups), then what filter_device does after its measure passes --
// u32 row pointers, the cells' offsets and tables in `cells` (whose host cell_group_off is not read).  A ref_id that is
// not below n_txps is no error here: out->bad_ref_record names the record (its index in d_records) and nothing else is
// filled; the caller knows the record's origin and writes the message.  Runs on the null stream and leaves it idle.
int filter_device_resident(const char *who, const oem_filters &F, const uint64_t *txp_len, uint32_t n_txps, const std::vector<float> &tab,
                           const oem_aln_record *d_records, const unsigned long long *d_group_off, uint64_t n_groups,
                           const unsigned long long *d_cell_group_off, bool want_coords, FilterResult *out, FilterCells *cells);
// The checks a device batch makes before any device use, and whether the host loop has to take it from the start
// (*host_only: no gap table for this score_prob_denom).
int filter_prepare_batch(const char *who, const oem_filters &F, const oem_aln_record *records, const uint64_t *group_off,
                         uint64_t n_groups, std::vector<float> *tab, bool *host_only);
// After a measure pass: the scans n_kept -> alignment offsets (aln_off) and n_kept > 0 -> row indices (row_idx), both of
// n_groups + 1 entries (out->n_kept has that many, the last one 0), out->nnz and out->n_rows from their ends, and the
// result's arrays allocated: row pointers (u32 when narrow, after checking base + nnz against 2^32; entry 0 = base), tid,
// as_prob and, with want_coords, start / end / strand.  Runs on the null stream and leaves it idle.  ev_begin / ev_end
// (or NULL) are recorded around the scans.
int filter_scan_alloc(const char *who, uint64_t n_groups, uint64_t base, bool want_coords, bool narrow, FilterResult *out,
                      DevBuf<uint64_t> *aln_off, DevBuf<uint64_t> *row_idx, hipEvent_t ev_begin, hipEvent_t ev_end);
// A pass's result (u64 row pointers, coordinates) appended to the builder, with out_kept and the discard table; atomic.
int filter_result_to_builder(oem_builder *b, FilterResult &r, uint64_t n_groups, uint32_t *out_kept);
// A pass's result (u32 row pointers; coordinates when model >= 0) made into a resident store, through the coverage
// model first when there is one: the tail of oem_store_create_records.  Consumes r.
int filter_result_to_store(const char *who, FilterResult &r, uint32_t n_txps, uint64_t n_groups, uint32_t bin_width, int model,
                           double growth_rate, int device, const oem_store_opts *opts, uint32_t *out_kept,
                           oem_discard_table *out_discard, oem_store **out);
// oem_filter_projected_device.hip -----------------------------------------------------------------------------------------
// What a projected batch of the records session keeps of the alignments k_proj_emit left unsure, instead of finishing
// them on the host batch by batch: n pairs (idx[i], f[i]) on the device, idx the alignment's index within the batch, in
// no particular order (k_proj_collect).  Their as_prob slots hold f until the session's finish has scattered expf(f).
struct ProjDeferred {
    DevBuf<uint64_t> idx;
    DevBuf<float> f;
    uint64_t n = 0;
};
// Measure, scans and emit of one projected batch on the current device: the body of
// oem_builder_add_projected_groups_device and oem_store_create_projected_records; the arguments are filter_device's plus
// the reads' lengths and the options (tab is read for OEM_PROJ_SCORE only).  An argument error found on the device
// (ref_id) is reported here.  deferred == NULL: the unsure alignments are finished on the host before the call returns.
// deferred != NULL (the session): they are collected into *deferred and left for proj_finish_deferred; under
// OEM_PROJ_SCORE the list is empty.  pinned_src: as filter_upload_measure.
int proj_device(const char *who, const oem_filters &F, const oem_proj_opts &P, const uint64_t *txp_len, uint32_t n_txps,
                const std::vector<float> &tab, const oem_proj_record *records, const uint64_t *group_off, const uint64_t *read_len,
                uint64_t n_groups, uint64_t base, bool want_coords, bool narrow, FilterResult *out, ProjDeferred *deferred = nullptr,
                bool pinned_src = false);
// Whether the host loop has to take every projected batch: no table for OEM_PROJ_SCORE (score_prob_denom; *tab is
// filled otherwise), a beta that is not finite for the two sources that use it.
bool proj_host_only(const oem_filters &F, const oem_proj_opts &P, std::vector<float> *tab);
// The deferred finish: n values f on the device come down, libm's expf goes back up and as_prob[idx[i]] = expf(f[i]).
// d_f is overwritten.  Leaves the null stream idle.
int proj_finish_deferred(const uint64_t *d_idx, float *d_f, uint64_t n, float *d_as_prob);

// The argument checks oem_store_create_records makes before any device use (shared by its projected counterpart).
int check_store_from_records(const char *who, const void *filters, const uint64_t *txp_len, uint32_t n_txps, uint32_t bin_width,
                             int model, const oem_store_opts *opts);

} // namespace oem
