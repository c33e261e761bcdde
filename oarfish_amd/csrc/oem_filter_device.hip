// oem_filter_device.hip -- AlignmentFilters::filter over a batch of reads on the device (SURVEY.md section 8f row 1,
// DESIGN.md section 5d): oem_builder_add_groups_device and oem_store_create_records.
//
// The per-group rule is oem_filter.h's, the same functions the host builder calls.  The call's floor is the upload of
// 40 B per record, so the kernels are kept simple.  Measured: the uploads run at the PCIe rate,
// the kernels and scans are under a fifth of the call, and what binds it is the staging copy described below.
//
//   upload            the records in chunks cut at group boundaries, from two pinned staging buffers, alternating between
//                     two streams: chunk k's k_filter_measure runs while chunk k + 1 is copied.  The records stay resident
//                     until the emit.  The caller's array is pageable, so every chunk is first copied into its staging
//                     buffer by the calling thread (one memcpy per chunk, under the other lane's DMA): a second pass over
//                     the records on the host, of the same order as the PCIe transfer, timed separately
//                     (filter_last_timing) and reported by scripts/filter_device_bench.py next to the upload.
//   k_filter_measure  one lane per group, the two walks of filter_group_measure: n_kept[g] and best[g], the group's
//                     contributions to the ten discard counters (summed over the wavefront, then one u64 atomicAdd per
//                     counter per wavefront), the ref_id and 2^24 flags
//   (hipcub scans)    n_kept -> alignment offsets, n_kept > 0 -> row indices
//   k_filter_emit     one lane per kept group: row_ptr, tid, as_prob (looked up in the host's expf table by the integer
//                     score gap: the device never computes exp), start, end, strand at the group's offsets
//
// The upload lanes, the scans and what is made of a pass's result (filter_result_to_builder, filter_result_to_store) are
// shared with the projected filter of oem_filter_projected_device.hip through oem_filter_device.h.
//
// oem_builder_add_groups_device copies the arrays back and appends them to the builder; oem_store_create_records frees
// the records and hands the arrays on as a ResidentCsr (model -1) or runs the coverage model on them first (0 / 1), as
// oem_store_create_coverage does after its upload.  Host arrays are brought back only for the host layout builder.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "oem_filter_device.h"

namespace oem {

namespace {

thread_local float g_filter_ms[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

// kPerCell (oem_cells_records.hip): the counters go to the lane's cell, cell_counts[cell * kFilterCounters + k], instead
// of tot->counts.  cell_group_off (n_cells + 1) holds the cells' first groups; the lane finds its cell by binary search.
// Groups are in cell order, so the lanes of a wavefront that share a cell are neighbours: a segmented sum over the
// wavefront leaves every cell's total in the first of its lanes, which issues the one u64 atomic per counter.
template <bool kPerCell>
__global__ __launch_bounds__(kFT) void k_filter_measure(oem_filters F, const oem_aln_record *__restrict__ recs,
                                                        const unsigned long long *__restrict__ group_off, uint64_t g0,
                                                        uint64_t g1, const uint64_t *__restrict__ txp_len, uint32_t n_txps,
                                                        uint32_t *__restrict__ n_kept, int32_t *__restrict__ best,
                                                        FilterTotals *__restrict__ tot,
                                                        const unsigned long long *__restrict__ cell_group_off, uint32_t n_cells,
                                                        unsigned long long *__restrict__ cell_counts)
{
    const uint64_t g = g0 + (uint64_t)blockIdx.x * kFT + threadIdx.x;
    FilterCounts c;
    if (g < g1) {
        const unsigned long long b = group_off[g], e = group_off[g + 1];
        const FilterGroup r = filter_group_measure(F, recs + b, (uint32_t)(e - b), txp_len, n_txps, c);
        n_kept[g] = r.n_kept;
        best[g] = r.best;
        if (r.flags) atomicOr(&tot->flags, r.flags);
        if (r.flags & kFilterFlagBadRef) atomicMin(&tot->bad_record, b + r.bad_record);
    }
    // every lane of the wavefront takes part (lanes past g1 add zeros)
    const uint32_t v[kFilterCounters] = {c.discard_5p, c.discard_3p, c.discard_score, c.discard_aln_frac, c.discard_aln_len,
                                         c.discard_ori, c.discard_supp, c.valid_best_aln, c.no_mapping, c.no_valid_aln};
    if constexpr (kPerCell) {
        const int lane = threadIdx.x & 63;
        uint32_t cell = 0xffffffffu; // (lanes past g1: a cell of their own, never written)
        if (g < g1) {
            uint32_t a = 0, b = n_cells; // the last cell whose first group is <= g (cells without groups share offsets)
            while (b - a > 1) {
                const uint32_t m = (a + b) >> 1;
                if (cell_group_off[m] <= g) a = m;
                else b = m;
            }
            cell = a;
        }
        const uint32_t before = __shfl_up(cell, 1);
        const bool head = lane == 0 || before != cell;
#pragma unroll
        for (int k = 0; k < kFilterCounters; ++k) {
            unsigned long long s = v[k];
            for (int off = 1; off < 64; off <<= 1) { // s = the sum over [lane, min(lane + 2 off, end of the cell's lanes))
                const unsigned long long t = __shfl_down(s, off);
                const uint32_t other = __shfl_down(cell, off);
                if (lane + off < 64 && other == cell) s += t;
            }
            if (head && s && cell != 0xffffffffu) atomicAdd(&cell_counts[(uint64_t)cell * kFilterCounters + k], s);
        }
    } else {
#pragma unroll
        for (int k = 0; k < kFilterCounters; ++k) {
            unsigned long long s = v[k];
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if ((threadIdx.x & 63) == 0 && s) atomicAdd(&tot->counts[k], s);
        }
    }
}

// One lane per cell boundary: the two scans sampled at the cells' first groups are the cells' first reads and first
// alignments in the filtered CSR.
__global__ __launch_bounds__(kFT) void k_filter_cell_offsets(const unsigned long long *__restrict__ cell_group_off, uint32_t n_cells,
                                                             const uint64_t *__restrict__ row_idx, const uint64_t *__restrict__ aln_off,
                                                             unsigned long long *__restrict__ cell_row_off,
                                                             unsigned long long *__restrict__ cell_aln_off)
{
    const uint32_t c = blockIdx.x * kFT + threadIdx.x;
    if (c > n_cells) return;
    const unsigned long long g = cell_group_off[c];
    cell_row_off[c] = row_idx[g];
    cell_aln_off[c] = aln_off[g];
}

// row_ptr64 or row_ptr32 (one of the two); start / end / strand may be NULL together (a store without a coverage model)
__global__ __launch_bounds__(kFT) void k_filter_emit(oem_filters F, const oem_aln_record *__restrict__ recs,
                                                     const unsigned long long *__restrict__ group_off, uint64_t n_groups,
                                                     const uint64_t *__restrict__ txp_len, uint32_t n_txps,
                                                     const uint32_t *__restrict__ n_kept, const int32_t *__restrict__ best,
                                                     const uint64_t *__restrict__ aln_off, const uint64_t *__restrict__ row_idx,
                                                     const float *__restrict__ tab, uint64_t n_tab, uint64_t base,
                                                     uint64_t *__restrict__ row_ptr64, uint32_t *__restrict__ row_ptr32,
                                                     uint32_t *__restrict__ tid, float *__restrict__ as_prob,
                                                     uint32_t *__restrict__ start, uint32_t *__restrict__ end,
                                                     uint8_t *__restrict__ strand)
{
    const uint64_t g = (uint64_t)blockIdx.x * kFT + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t k = n_kept[g];
    if (k == 0) return;
    const uint64_t o = aln_off[g], r = row_idx[g];
    if (row_ptr64) row_ptr64[r + 1] = base + o + k;
    else row_ptr32[r + 1] = (uint32_t)(base + o + k);
    const unsigned long long b = group_off[g], e = group_off[g + 1];
    filter_group_emit(F, recs + b, (uint32_t)(e - b), txp_len, n_txps, best[g],
                      [&](uint32_t q, uint32_t, const oem_aln_record &x, uint64_t gap) {
                          const uint64_t j = o + q;
                          tid[j] = x.ref_id;
                          as_prob[j] = filter_prob(tab, n_tab, gap);
                          if (start) {
                              start[j] = x.aln_start;
                              end[j] = x.aln_end;
                              strand[j] = (x.flags & OEM_REC_REVERSE) ? 1 : 0;
                          }
                      });
}

struct U32ToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};
struct NonZeroToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v ? 1 : 0; }
};

// What follows a measure pass that found nothing to report: the tables, the two scans, the cells' offsets and the emit.
// d_cgo / d_ccnt: the per-cell form's device arrays (with `cells`).
int filter_scans_emit(const char *who, const oem_filters &F, uint32_t n_txps, const std::vector<float> &tab,
                      const oem_aln_record *d_recs, const unsigned long long *d_goff, uint64_t n_groups, uint64_t base,
                      bool want_coords, bool narrow, FilterResult *out, FilterCells *cells, const unsigned long long *d_cgo,
                      const unsigned long long *d_ccnt, const int32_t *d_best, const FilterTotals &h_tot, bool timing)
{
    const uint32_t n_cells = cells ? cells->n_cells : 0;
    DevBuf<uint64_t> d_aln_off, d_row_idx;
    DevBuf<float> d_tab;
    const uint64_t *cnt = (const uint64_t *)h_tot.counts;
    out->dt = oem_discard_table{cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], cnt[5], cnt[6], cnt[7], cnt[8], cnt[9]};
    if (cells) { // the cells' tables; the batch's is their sum
        cells->tables.assign(n_cells, oem_discard_table{});
        if (n_cells)
            OEM_HIP(hipMemcpy(cells->tables.data(), d_ccnt, sizeof(oem_discard_table) * n_cells, hipMemcpyDeviceToHost));
        uint64_t *sum = &out->dt.discard_5p;
        for (const oem_discard_table &t : cells->tables)
            for (int k = 0; k < kFilterCounters; ++k) sum[k] += (&t.discard_5p)[k];
    }

    // -- scans, emit ---------------------------------------------------------------------------------------------------
    hipStream_t st = nullptr; // the emit follows the scans on the null stream (the lanes are idle)
    Event ev[3];
    if (timing)
        for (auto &e : ev) OEM_HIP(hipEventCreate(&e.e));
    OEM_TRY(filter_scan_alloc(who, n_groups, base, want_coords, narrow, out, &d_aln_off, &d_row_idx, ev[0].e, ev[1].e));
    const uint64_t nnz = out->nnz;
    if (cells) {
        OEM_TRY(dev_alloc(&cells->d_cell_row_off.p, (size_t)n_cells + 1, nullptr));
        OEM_TRY(dev_alloc(&cells->d_cell_aln_off.p, (size_t)n_cells + 1, nullptr));
        hipLaunchKernelGGL(k_filter_cell_offsets, dim3((n_cells + 1 + kFT - 1) / kFT), dim3(kFT), 0, st, d_cgo, n_cells,
                           d_row_idx.p, d_aln_off.p, cells->d_cell_row_off.p, cells->d_cell_aln_off.p);
        OEM_HIP(hipGetLastError());
        cells->cell_row_off.resize((size_t)n_cells + 1);
        cells->cell_aln_off.resize((size_t)n_cells + 1);
        OEM_HIP(hipMemcpyAsync(cells->cell_row_off.data(), cells->d_cell_row_off.p, sizeof(uint64_t) * ((size_t)n_cells + 1), hipMemcpyDeviceToHost, st));
        OEM_HIP(hipMemcpyAsync(cells->cell_aln_off.data(), cells->d_cell_aln_off.p, sizeof(uint64_t) * ((size_t)n_cells + 1), hipMemcpyDeviceToHost, st));
    }
    OEM_TRY(dev_alloc(&d_tab.p, tab.size(), nullptr));
    if (!tab.empty()) OEM_HIP(hipMemcpy(d_tab.p, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    if (n_groups && nnz) {
        hipLaunchKernelGGL(k_filter_emit, dim3((uint32_t)((n_groups + kFT - 1) / kFT)), dim3(kFT), 0, st, F, d_recs, d_goff,
                           n_groups, out->txp_len.p, n_txps, out->n_kept.p, d_best, d_aln_off.p, d_row_idx.p, d_tab.p,
                           (uint64_t)tab.size(), base, out->row_ptr64.p, out->row_ptr32.p, out->tid.p, out->as_prob.p,
                           out->start.p, out->end.p, out->strand.p);
        OEM_HIP(hipGetLastError());
    }
    if (timing) OEM_HIP(hipEventRecord(ev[2].e, st));
    OEM_HIP(hipStreamSynchronize(st));
    if (timing) {
        OEM_HIP(hipEventElapsedTime(&g_filter_ms[2], ev[0].e, ev[1].e));
        OEM_HIP(hipEventElapsedTime(&g_filter_ms[3], ev[1].e, ev[2].e));
    }
    return OEM_OK; // (the scan results are released here, the records and offsets with the caller's scope)
}

} // namespace

int filter_device(const char *who, const oem_filters &F, const uint64_t *txp_len, uint32_t n_txps, const std::vector<float> &tab,
                  const oem_aln_record *records, const uint64_t *group_off, uint64_t n_groups, uint64_t base, bool want_coords,
                  bool narrow, FilterResult *out, FilterCells *cells, bool pinned_src)
{
    const bool timing = knob("OEM_FILTER_TIMING", 0) != 0;
    const uint64_t n_records = group_off[n_groups];
    const uint64_t chunk = (uint64_t)filter_chunk_groups();

    DevBuf<oem_aln_record> d_recs;
    DevBuf<unsigned long long> d_goff;
    DevBuf<int32_t> d_best;
    DevBuf<FilterTotals> d_tot;
    DevBuf<unsigned long long> d_cgo, d_ccnt; // the per-cell form: the cells' first groups, their counters
    const uint32_t n_cells = cells ? cells->n_cells : 0;
    if (cells) {
        OEM_TRY(dev_alloc(&d_cgo.p, (size_t)n_cells + 1, nullptr));
        OEM_TRY(dev_alloc(&d_ccnt.p, (size_t)n_cells * kFilterCounters, nullptr));
        OEM_HIP(hipMemcpy(d_cgo.p, cells->cell_group_off, sizeof(uint64_t) * ((size_t)n_cells + 1), hipMemcpyHostToDevice));
        OEM_HIP(hipMemset(d_ccnt.p, 0, sizeof(uint64_t) * (n_cells ? (size_t)n_cells * kFilterCounters : 1)));
    }
    OEM_TRY(dev_alloc(&d_recs.p, n_records, nullptr));
    OEM_TRY(dev_alloc(&d_goff.p, n_groups + 1, nullptr));
    OEM_TRY(dev_alloc(&out->n_kept.p, n_groups + 1, nullptr));
    OEM_TRY(dev_alloc(&d_best.p, n_groups + 1, nullptr));
    OEM_TRY(dev_alloc(&d_tot.p, 1, nullptr));
    OEM_TRY(dev_alloc(&out->txp_len.p, n_txps, nullptr));
    FilterTotals h_tot;
    std::memset(&h_tot, 0, sizeof(h_tot));
    h_tot.bad_record = kNoRecord;
    OEM_HIP(hipMemcpy(d_tot.p, &h_tot, sizeof(h_tot), hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_goff.p, group_off, sizeof(uint64_t) * (n_groups + 1), hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(out->txp_len.p, txp_len, sizeof(uint64_t) * n_txps, hipMemcpyHostToDevice));
    OEM_HIP(hipMemset(out->n_kept.p + n_groups, 0, sizeof(uint32_t))); // (the scans read n_groups + 1 entries)
    OEM_HIP(hipStreamSynchronize(nullptr)); // (the lanes below do not wait for the null stream)

    // -- upload + measure ----------------------------------------------------------------------------------------------
    OEM_TRY(filter_upload_measure(records, d_recs.p, group_off, n_groups, chunk, timing ? g_filter_ms : nullptr,
                                  [&](hipStream_t st, uint64_t g0, uint64_t g1) {
                                      const dim3 grid((uint32_t)((g1 - g0 + kFT - 1) / kFT));
                                      if (cells)
                                          hipLaunchKernelGGL(k_filter_measure<true>, grid, dim3(kFT), 0, st, F, d_recs.p, d_goff.p, g0,
                                                             g1, out->txp_len.p, n_txps, out->n_kept.p, d_best.p, d_tot.p, d_cgo.p,
                                                             n_cells, d_ccnt.p);
                                      else
                                          hipLaunchKernelGGL(k_filter_measure<false>, grid, dim3(kFT), 0, st, F, d_recs.p, d_goff.p, g0,
                                                             g1, out->txp_len.p, n_txps, out->n_kept.p, d_best.p, d_tot.p, nullptr, 0u,
                                                             nullptr);
                                  },
                                  pinned_src));
    OEM_HIP(hipMemcpy(&h_tot, d_tot.p, sizeof(h_tot), hipMemcpyDeviceToHost));
    if (h_tot.flags & kFilterFlagBadRef) {
        if (!cells)
            return fail(OEM_ERR_ARG, "%s: record %llu: ref_id %u is not below n_txps", who, h_tot.bad_record,
                        records[h_tot.bad_record].ref_id);
        // the record's group, then the group's cell (the last one that starts at or before it)
        const uint64_t g = (uint64_t)(std::upper_bound(group_off, group_off + n_groups + 1, (uint64_t)h_tot.bad_record) - group_off) - 1;
        const uint64_t c = (uint64_t)(std::upper_bound(cells->cell_group_off, cells->cell_group_off + n_cells + 1, g) - cells->cell_group_off) - 1;
        return fail(OEM_ERR_ARG, "%s: cell %llu: record %llu: ref_id %u is not below n_txps", who,
                    (unsigned long long)(cells->first_cell + c), (unsigned long long)(cells->first_record + h_tot.bad_record),
                    records[h_tot.bad_record].ref_id);
    }
    if (h_tot.flags & kFilterFlagBigScore) {
        out->host_rerun = true;
        return OEM_OK;
    }
    return filter_scans_emit(who, F, n_txps, tab, d_recs.p, d_goff.p, n_groups, base, want_coords, narrow, out, cells, d_cgo.p, d_ccnt.p,
                             d_best.p, h_tot, timing);
}

// The resident form (oem_filter_device.h): no upload lanes, one measure launch over all groups.
int filter_device_resident(const char *who, const oem_filters &F, const uint64_t *txp_len, uint32_t n_txps, const std::vector<float> &tab,
                           const oem_aln_record *d_records, const unsigned long long *d_group_off, uint64_t n_groups,
                           const unsigned long long *d_cell_group_off, bool want_coords, FilterResult *out, FilterCells *cells)
{
    const bool timing = knob("OEM_FILTER_TIMING", 0) != 0;
    const uint32_t n_cells = cells->n_cells;
    hipStream_t st = nullptr;
    DevBuf<int32_t> d_best;
    DevBuf<FilterTotals> d_tot;
    DevBuf<unsigned long long> d_ccnt;
    OEM_TRY(dev_alloc(&d_ccnt.p, (size_t)n_cells * kFilterCounters, nullptr));
    OEM_TRY(dev_alloc(&out->n_kept.p, n_groups + 1, nullptr));
    OEM_TRY(dev_alloc(&d_best.p, n_groups + 1, nullptr));
    OEM_TRY(dev_alloc(&d_tot.p, 1, nullptr));
    OEM_TRY(dev_alloc(&out->txp_len.p, n_txps, nullptr));
    FilterTotals h_tot;
    std::memset(&h_tot, 0, sizeof(h_tot));
    h_tot.bad_record = kNoRecord;
    OEM_HIP(hipMemset(d_ccnt.p, 0, sizeof(uint64_t) * (n_cells ? (size_t)n_cells * kFilterCounters : 1)));
    OEM_HIP(hipMemcpy(d_tot.p, &h_tot, sizeof(h_tot), hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(out->txp_len.p, txp_len, sizeof(uint64_t) * n_txps, hipMemcpyHostToDevice));
    OEM_HIP(hipMemset(out->n_kept.p + n_groups, 0, sizeof(uint32_t))); // (the scans read n_groups + 1 entries)
    if (n_groups) {
        hipLaunchKernelGGL(k_filter_measure<true>, dim3((uint32_t)((n_groups + kFT - 1) / kFT)), dim3(kFT), 0, st, F, d_records,
                           d_group_off, (uint64_t)0, n_groups, out->txp_len.p, n_txps, out->n_kept.p, d_best.p, d_tot.p,
                           d_cell_group_off, n_cells, d_ccnt.p);
        OEM_HIP(hipGetLastError());
    }
    OEM_HIP(hipMemcpy(&h_tot, d_tot.p, sizeof(h_tot), hipMemcpyDeviceToHost));
    if (h_tot.flags & kFilterFlagBadRef) { // the caller knows where the record came from: it writes the message
        out->bad_ref_record = h_tot.bad_record;
        return OEM_OK;
    }
    if (h_tot.flags & kFilterFlagBigScore) {
        out->host_rerun = true;
        return OEM_OK;
    }
    return filter_scans_emit(who, F, n_txps, tab, d_records, d_group_off, n_groups, 0, want_coords, true, out, cells, d_cell_group_off,
                             d_ccnt.p, d_best.p, h_tot, timing);
}

int filter_prepare_batch(const char *who, const oem_filters &F, const oem_aln_record *records, const uint64_t *group_off,
                  uint64_t n_groups, std::vector<float> *tab, bool *host_only)
{
    OEM_TRY(check_group_off(who, records, group_off, n_groups));
    if (n_groups >= 0x7fffffffull) return fail(OEM_ERR_ARG, "%s: at most 2^31 - 2 groups per call", who);
    *host_only = !filter_prob_table(F.score_prob_denom, *tab);
    return OEM_OK;
}

namespace {

// host arrays for the host layout builder, fetched from the store that adopted the resident CSR
struct HostCsr {
    oem_store *s = nullptr;
    std::vector<uint64_t> row_ptr;
    std::vector<uint32_t> tid;
    static const uint64_t *get_row_ptr(void *ctx)
    {
        HostCsr *h = (HostCsr *)ctx;
        try {
            std::vector<uint32_t> rp32(h->s->csr.n_reads + 1);
            if (hipMemcpy(rp32.data(), h->s->csr.row_ptr, sizeof(uint32_t) * rp32.size(), hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
            h->row_ptr.assign(rp32.begin(), rp32.end());
        } catch (...) {
            return nullptr;
        }
        return h->row_ptr.data();
    }
    static const uint32_t *get_tid(void *ctx)
    {
        HostCsr *h = (HostCsr *)ctx;
        try {
            h->tid.resize(h->s->csr.nnz ? h->s->csr.nnz : 1);
            if (h->s->csr.nnz && hipMemcpy(h->tid.data(), h->s->csr.tid, sizeof(uint32_t) * h->s->csr.nnz, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
        } catch (...) {
            return nullptr;
        }
        return h->tid.data();
    }
};

} // namespace

void filter_last_timing(float *ms6) { std::memcpy(ms6, g_filter_ms, sizeof g_filter_ms); }
void filter_timing_reset() { for (float &m : g_filter_ms) m = 0.f; }

int filter_scan_alloc(const char *who, uint64_t n_groups, uint64_t base, bool want_coords, bool narrow, FilterResult *out,
                      DevBuf<uint64_t> *aln_off, DevBuf<uint64_t> *row_idx, hipEvent_t ev_begin, hipEvent_t ev_end)
{
    hipStream_t st = nullptr;
    OEM_TRY(dev_alloc(&aln_off->p, n_groups + 1, nullptr));
    OEM_TRY(dev_alloc(&row_idx->p, n_groups + 1, nullptr));
    if (ev_begin) OEM_HIP(hipEventRecord(ev_begin, st));
    {
        hipcub::TransformInputIterator<uint64_t, U32ToU64, const uint32_t *> in_a(out->n_kept.p, U32ToU64());
        hipcub::TransformInputIterator<uint64_t, NonZeroToU64, const uint32_t *> in_r(out->n_kept.p, NonZeroToU64());
        size_t tmp_a = 0, tmp_r = 0;
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_a, in_a, aln_off->p, (int)(n_groups + 1), st));
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_r, in_r, row_idx->p, (int)(n_groups + 1), st));
        DevBuf<uint8_t> d_tmp;
        OEM_TRY(dev_alloc(&d_tmp.p, tmp_a > tmp_r ? tmp_a : tmp_r, nullptr));
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_a, in_a, aln_off->p, (int)(n_groups + 1), st));
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_r, in_r, row_idx->p, (int)(n_groups + 1), st));
        OEM_HIP(hipStreamSynchronize(st));
    }
    if (ev_end) OEM_HIP(hipEventRecord(ev_end, st));
    uint64_t nnz = 0, n_rows = 0;
    OEM_HIP(hipMemcpy(&nnz, aln_off->p + n_groups, sizeof(nnz), hipMemcpyDeviceToHost));
    OEM_HIP(hipMemcpy(&n_rows, row_idx->p + n_groups, sizeof(n_rows), hipMemcpyDeviceToHost));
    if (narrow && base + nnz >= (1ull << 32))
        return fail(OEM_ERR_ARG, "%s: %llu alignments are kept; a resident store needs fewer than 2^32", who, (unsigned long long)nnz);
    out->nnz = nnz;
    out->n_rows = n_rows;
    if (narrow) {
        OEM_TRY(dev_alloc(&out->row_ptr32.p, n_rows + 1, nullptr));
        const uint32_t b32 = (uint32_t)base;
        OEM_HIP(hipMemcpy(out->row_ptr32.p, &b32, sizeof(b32), hipMemcpyHostToDevice));
    } else {
        OEM_TRY(dev_alloc(&out->row_ptr64.p, n_rows + 1, nullptr));
        OEM_HIP(hipMemcpy(out->row_ptr64.p, &base, sizeof(base), hipMemcpyHostToDevice));
    }
    OEM_TRY(dev_alloc(&out->tid.p, nnz, nullptr));
    OEM_TRY(dev_alloc(&out->as_prob.p, nnz, nullptr));
    if (want_coords) {
        OEM_TRY(dev_alloc(&out->start.p, nnz, nullptr));
        OEM_TRY(dev_alloc(&out->end.p, nnz, nullptr));
        OEM_TRY(dev_alloc(&out->strand.p, nnz, nullptr));
    }
    return OEM_OK;
}

int filter_result_to_builder(oem_builder *b, FilterResult &r, uint64_t n_groups, uint32_t *out_kept)
{
    const BuilderMark mark = builder_mark(b);
    int rc = OEM_OK;
    try {
        b->row_ptr.resize(mark.n_row_ptr + r.n_rows);
        b->tid.resize(mark.nnz + r.nnz);
        b->as_prob.resize(mark.nnz + r.nnz);
        b->start.resize(mark.nnz + r.nnz);
        b->end.resize(mark.nnz + r.nnz);
        b->strand.resize(mark.nnz + r.nnz);
        auto back = [&](void *dst, const void *src, size_t bytes) -> int {
            if (bytes) OEM_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
            return OEM_OK;
        };
        rc = back(b->row_ptr.data() + mark.n_row_ptr, r.row_ptr64.p + 1, sizeof(uint64_t) * r.n_rows);
        if (rc == OEM_OK) rc = back(b->tid.data() + mark.nnz, r.tid.p, sizeof(uint32_t) * r.nnz);
        if (rc == OEM_OK) rc = back(b->as_prob.data() + mark.nnz, r.as_prob.p, sizeof(float) * r.nnz);
        if (rc == OEM_OK) rc = back(b->start.data() + mark.nnz, r.start.p, sizeof(uint32_t) * r.nnz);
        if (rc == OEM_OK) rc = back(b->end.data() + mark.nnz, r.end.p, sizeof(uint32_t) * r.nnz);
        if (rc == OEM_OK) rc = back(b->strand.data() + mark.nnz, r.strand.p, r.nnz);
        if (rc == OEM_OK && out_kept) rc = back(out_kept, r.n_kept.p, sizeof(uint32_t) * n_groups);
    } catch (...) {
        builder_rollback(b, mark);
        throw;
    }
    if (rc != OEM_OK) {
        builder_rollback(b, mark);
        return rc;
    }
    const uint64_t *add = &r.dt.discard_5p;
    uint64_t *dt = &b->dt.discard_5p;
    for (int k = 0; k < kFilterCounters; ++k) dt[k] += add[k];
    return OEM_OK;
}

int check_store_from_records(const char *who, const void *filters, const uint64_t *txp_len, uint32_t n_txps, uint32_t bin_width,
                             int model, const oem_store_opts *opts)
{
    if (!filters || !txp_len || n_txps == 0) return fail(OEM_ERR_ARG, "%s: bad argument", who);
    if (model < -1 || model > 1) return fail(OEM_ERR_ARG, "%s: model must be -1 (none), 0 (logistic) or 1 (binomial)", who);
    if (model >= 0 && bin_width == 0)
        return fail(OEM_ERR_ARG, "coverage model with 0 bin width is not implemented (logistic_probability.rs:59, binomial_probability.rs:192)");
    if (opts && opts->weight_coding > 2) return fail(OEM_ERR_ARG, "%s: weight_coding %u (0, 1 or 2)", who, opts->weight_coding);
    if (opts && opts->layout_build > 1) return fail(OEM_ERR_ARG, "%s: layout_build %u (0 or 1)", who, opts->layout_build);
    if (opts && opts->reorder_rows > 2) return fail(OEM_ERR_ARG, "%s: reorder_rows %u (0, 1 or 2)", who, opts->reorder_rows);
    return OEM_OK;
}

int filter_result_to_store(const char *who, FilterResult &r, uint32_t n_txps, uint64_t n_groups, uint32_t bin_width, int model,
                           double growth_rate, int device, const oem_store_opts *opts, uint32_t *out_kept,
                           oem_discard_table *out_discard, oem_store **out)
{
    if (out_kept && n_groups) OEM_HIP(hipMemcpy(out_kept, r.n_kept.p, sizeof(uint32_t) * n_groups, hipMemcpyDeviceToHost));
    if (out_discard) *out_discard = r.dt;
    r.n_kept.reset();

    // weight_coding 2 (create_store_impl refuses it on a resident CSR): with a coverage model the products are rounded
    // once into w32 and the store is asked for coding 1; without one it is coding 0
    oem_store_opts o;
    std::memset(&o, 0, sizeof(o));
    if (opts) o = *opts;
    const bool f32w = model >= 0 && o.weight_coding == 2;
    if (o.weight_coding == 2) o.weight_coding = model >= 0 ? 1u : 0u;

    ResidentCsr res;
    res.row_ptr = r.row_ptr32.p;
    r.row_ptr32.p = nullptr;
    res.tid = r.tid.p;
    r.tid.p = nullptr;
    if (model < 0) {
        res.w32 = r.as_prob.p;
        r.as_prob.p = nullptr;
    } else {
        if (f32w) OEM_TRY(dev_alloc(&res.w32, r.nnz, nullptr));
        else OEM_TRY(dev_alloc(&res.w64, r.nnz, nullptr));
        if (r.nnz) {
            DevBuf<double> d_cov;
            OEM_TRY(dev_alloc(&d_cov.p, r.nnz, nullptr));
            OEM_TRY(coverage_resident(res.row_ptr, res.tid, r.start.p, r.end.p, r.txp_len.p, r.n_rows, r.nnz, n_txps, bin_width,
                                      model, growth_rate, d_cov.p, r.as_prob.p, res.w64, res.w32));
        }
        r.as_prob.reset();
        r.start.reset();
        r.end.reset();
        r.strand.reset();
    }
    r.txp_len.reset();

    oem_store *s = new (std::nothrow) oem_store();
    if (!s) return fail(OEM_ERR_OOM, "%s: host allocation failed", who);
    HostCsr host;
    host.s = s;
    res.host_row_ptr = &HostCsr::get_row_ptr;
    res.host_tid = &HostCsr::get_tid;
    res.host_row_ptr_ctx = &host;
    const uint64_t *h_rp = nullptr;
    const uint32_t *h_tid = nullptr;
    std::vector<uint64_t> rp64;
    std::vector<uint32_t> tid32;
    if (o.layout_build == 1) { // the host layout builder reads host arrays: bring them back, then and only then
        std::vector<uint32_t> rp32(r.n_rows + 1);
        tid32.resize(r.nnz ? r.nnz : 1);
        hipError_t e = hipMemcpy(rp32.data(), res.row_ptr, sizeof(uint32_t) * rp32.size(), hipMemcpyDeviceToHost);
        if (e == hipSuccess && r.nnz) e = hipMemcpy(tid32.data(), res.tid, sizeof(uint32_t) * r.nnz, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            free_store(s);
            return fail(OEM_ERR_HIP, "%s: reading the CSR back failed: %s", who, hipGetErrorString(e));
        }
        rp64.assign(rp32.begin(), rp32.end());
        h_rp = rp64.data();
        h_tid = tid32.data();
    }
    const int rc = create_store_impl(h_rp, h_tid, nullptr, nullptr, r.n_rows, r.nnz, n_txps, device, &o, s, nullptr, &res);
    if (rc != OEM_OK) {
        free_store(s);
        return rc;
    }
    *out = s;
    return OEM_OK;
}

} // namespace oem

using namespace oem;

extern "C" int oem_builder_add_groups_device(oem_builder *b, const oem_aln_record *records, const uint64_t *group_off,
                                             uint64_t n_groups, int device, uint32_t *out_kept)
{
    OEM_API_BEGIN
    const char *who = "oem_builder_add_groups_device";
    filter_timing_reset();
    if (!b) return fail(OEM_ERR_ARG, "%s: builder is NULL", who);
    std::vector<float> tab;
    bool host_only = false;
    OEM_TRY(filter_prepare_batch(who, b->f, records, group_off, n_groups, &tab, &host_only));
    OEM_TRY(ensure_device(device));
    if (host_only) return add_groups_host(b, records, group_off, n_groups, out_kept, who);
    FilterResult r;
    const uint64_t base = b->tid.size();
    OEM_TRY(filter_device(who, b->f, b->txp_len.data(), (uint32_t)b->txp_len.size(), tab, records, group_off, n_groups, base,
                          true, false, &r));
    if (r.host_rerun) return add_groups_host(b, records, group_off, n_groups, out_kept, who);
    return filter_result_to_builder(b, r, n_groups, out_kept);
    OEM_API_END("oem_builder_add_groups_device")
}

extern "C" int oem_store_create_records(const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                                        const oem_aln_record *records, const uint64_t *group_off, uint64_t n_groups,
                                        uint32_t bin_width, int model, double growth_rate, int device,
                                        const oem_store_opts *opts, uint32_t *out_kept, oem_discard_table *out_discard,
                                        oem_store **out)
{
    OEM_API_BEGIN
    const char *who = "oem_store_create_records";
    filter_timing_reset();
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    OEM_TRY(check_store_from_records(who, filters, txp_len, n_txps, bin_width, model, opts));
    std::vector<float> tab;
    bool host_only = false;
    OEM_TRY(filter_prepare_batch(who, *filters, records, group_off, n_groups, &tab, &host_only));
    OEM_TRY(ensure_device(device));

    FilterResult r;
    if (!host_only)
        OEM_TRY(filter_device(who, *filters, txp_len, n_txps, tab, records, group_off, n_groups, 0, model >= 0, true, &r));
    if (host_only || r.host_rerun) { // the host loop takes the batch: the long way round, same store
        oem_builder hb;
        hb.f = *filters;
        hb.txp_len.assign(txp_len, txp_len + n_txps);
        OEM_TRY(add_groups_host(&hb, records, group_off, n_groups, out_kept, who));
        if (hb.tid.size() >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: a resident store needs fewer than 2^32 alignments", who);
        if (out_discard) *out_discard = hb.dt;
        if (model < 0) return oem_builder_store_create(&hb, nullptr, device, opts, out);
        return oem_builder_store_create_coverage(&hb, bin_width, model, growth_rate, device, opts, nullptr, out);
    }
    return filter_result_to_store(who, r, n_txps, n_groups, bin_width, model, growth_rate, device, opts, out_kept, out_discard, out);
    OEM_API_END("oem_store_create_records")
}
