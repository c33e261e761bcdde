// oem_filter_projected_device.hip -- AlignmentFilters::filter_projected over a batch of genome-mode reads on the device
// (DESIGN.md section 5d): oem_builder_add_projected_groups_device and
// oem_store_create_projected_records.
//
// The per-group rule is oem_filter_projected.h's, the same functions the host builder calls; the pass has the shape of
// oem_filter_device.hip's and shares its upload lanes, scans and tails (oem_filter_device.h):
//
//   upload            as there: 40 B per record in chunks cut at group boundaries, two lanes
//   k_proj_measure    one lane per group, the two walks of proj_group_measure: n_kept[g], best_sim[g], best_score[g], the
//                     group's contributions to the discard counters (summed over the wavefront, one u64 atomicAdd per
//                     counter per wavefront), the argument-error and 2^24 flags
//   (hipcub scans)    n_kept -> alignment offsets, n_kept > 0 -> row indices
//   k_proj_emit       one lane per kept group: row_ptr, tid, clamped start / end, strand, and as_prob
//   finish            OEM_PROJ_SIMILARITY / _COMBINED only, see below
//
// as_prob.  OEM_PROJ_SCORE looks it up in the host's expf table by the integer score gap, exactly as k_filter_emit does.
// For the other two sources the argument f is a continuous f32, and expf is by definition the host libm's, which no
// device exponential equals everywhere.  k_proj_emit writes exp_f32_candidate(f) (oem_exp_f32.h) where that is provably
// what a libm expf returns; where it is not (f not finite or positive, a subnormal result, an f64 value within 1/256 ulp
// of a rounding tie: about 0.4 % of the alignments) it writes f itself into the as_prob slot and sets the alignment's
// flag.  The flagged (index, f) pairs are compacted with hipcub::DeviceSelect::Flagged and copied down, the host applies
// expf, the values go back up and k_proj_scatter stores them -- before the arrays are handed to the builder, the coverage
// model or the layout build.  The records session (oem_records_stream.hip) does not finish batch by batch: its batches
// keep their (index, f) pairs on the device (k_proj_collect, a wavefront ballot instead of the select passes) and its
// finish runs the host's expf once over all of them (proj_finish_deferred).
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstring>
#include <vector>

#include "oem_exp_f32.h"
#include "oem_filter_device.h"
#include "oem_filter_projected.h"

namespace oem {

namespace {

// this thread's last call: ms of k_proj_measure, of k_proj_emit, of the finish; alignments finished by the host, emitted
thread_local double g_proj_pass[5] = {0., 0., 0., 0., 0.};

__global__ __launch_bounds__(kFT) void k_proj_measure(oem_filters F, const oem_proj_record *__restrict__ recs,
                                                      const unsigned long long *__restrict__ group_off,
                                                      const uint64_t *__restrict__ read_len, uint64_t g0, uint64_t g1,
                                                      const uint64_t *__restrict__ txp_len, uint32_t n_txps,
                                                      uint32_t *__restrict__ n_kept, double *__restrict__ best_sim,
                                                      int32_t *__restrict__ best_score, FilterTotals *__restrict__ tot)
{
    const uint64_t g = g0 + (uint64_t)blockIdx.x * kFT + threadIdx.x;
    FilterCounts c;
    if (g < g1) {
        const unsigned long long b = group_off[g], e = group_off[g + 1];
        const ProjGroup r = proj_group_measure(F, recs + b, (uint32_t)(e - b), read_len[g], txp_len, n_txps, c);
        n_kept[g] = r.n_kept;
        best_sim[g] = r.best_sim;
        best_score[g] = r.best_score;
        if (r.flags) atomicOr(&tot->flags, r.flags);
        if (r.flags & kFilterFlagBadRef) atomicMin(&tot->bad_record, b + r.bad_record);
    }
    // every lane of the wavefront takes part (lanes past g1 add zeros); discard_supp, no_mapping and no_valid_aln stay
    // zero, filter_projected never counts them
    const uint32_t v[kFilterCounters] = {c.discard_5p, c.discard_3p, c.discard_score, c.discard_aln_frac, c.discard_aln_len,
                                         c.discard_ori, c.discard_supp, c.valid_best_aln, c.no_mapping, c.no_valid_aln};
#pragma unroll
    for (int k = 0; k < kFilterCounters; ++k) {
        unsigned long long s = v[k];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&tot->counts[k], s);
    }
}

// row_ptr64 or row_ptr32 (one of the two); start / end / strand may be NULL together (a store without a coverage model).
// tab != NULL: OEM_PROJ_SCORE, as_prob from the table.  Otherwise the candidate, or f and unsure[j] = 1.
__global__ __launch_bounds__(kFT) void k_proj_emit(oem_filters F, oem_proj_opts P, const oem_proj_record *__restrict__ recs,
                                                   const unsigned long long *__restrict__ group_off, uint64_t n_groups,
                                                   const uint64_t *__restrict__ txp_len, uint32_t n_txps,
                                                   const uint32_t *__restrict__ n_kept, const double *__restrict__ best_sim,
                                                   const int32_t *__restrict__ best_score, const uint64_t *__restrict__ aln_off,
                                                   const uint64_t *__restrict__ row_idx, const float *__restrict__ tab,
                                                   uint64_t n_tab, uint64_t base, uint64_t *__restrict__ row_ptr64,
                                                   uint32_t *__restrict__ row_ptr32, uint32_t *__restrict__ tid,
                                                   float *__restrict__ as_prob, uint8_t *__restrict__ unsure,
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
    const int32_t bs = best_score[g];
    proj_group_emit(F, P, recs + b, (uint32_t)(e - b), txp_len, n_txps, best_sim[g], bs,
                    [&](uint32_t q, uint32_t, const oem_proj_record &x, uint32_t s, uint32_t en, float f) {
                        const uint64_t j = o + q;
                        tid[j] = x.ref_id;
                        if (tab) {
                            as_prob[j] = filter_prob(tab, n_tab, proj_gap(bs, x));
                        } else {
                            bool sure;
                            const float c = exp_f32_candidate(f, &sure);
                            as_prob[j] = sure ? c : f;
                            unsure[j] = sure ? 0 : 1;
                        }
                        if (start) {
                            start[j] = s;
                            end[j] = en;
                            strand[j] = (x.flags & OEM_REC_REVERSE) ? 1 : 0;
                        }
                    });
}

__global__ __launch_bounds__(kFT) void k_proj_scatter(const uint64_t *__restrict__ idx, const float *__restrict__ val, uint64_t n,
                                                      float *__restrict__ as_prob)
{
    const uint64_t i = (uint64_t)blockIdx.x * kFT + threadIdx.x;
    if (i < n) as_prob[idx[i]] = val[i];
}

// The session's form of the compaction ("The projected session"): one lane per alignment of a
// batch's piece.  A wavefront takes the ballot of its lanes' flags, its first lane reserves that many entries of the
// piece's list with one atomicAdd, and the flagged lanes store (piece-local index, f) behind one another.  The list's
// order is whatever order the wavefronts arrive in: indices are distinct and the later scatter is by index.  No lane
// leaves before the ballot, so lane 0 always holds the reservation.
__global__ __launch_bounds__(kFT) void k_proj_collect(const uint8_t *__restrict__ unsure, const float *__restrict__ as_prob, uint64_t nnz,
                                                      unsigned long long *__restrict__ count, uint64_t *__restrict__ idx,
                                                      float *__restrict__ f)
{
    const uint64_t j = (uint64_t)blockIdx.x * kFT + threadIdx.x;
    const bool flagged = j < nnz && unsure[j] != 0;
    const unsigned long long votes = __ballot(flagged);
    if (votes == 0) return; // (uniform over the wavefront)
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long first = 0;
    if (lane == 0) first = atomicAdd(count, (unsigned long long)__popcll(votes));
    first = __shfl(first, 0);
    if (flagged) {
        const uint64_t at = first + (uint64_t)__popcll(votes & ((1ull << lane) - 1));
        idx[at] = j;
        f[at] = as_prob[j];
    }
}

// The batch's unsure alignments into *d: k_proj_collect into lists of nnz entries, the count down, the lists cut to size.
int collect_deferred(const float *d_as_prob, const uint8_t *d_unsure, uint64_t nnz, ProjDeferred *d)
{
    d->n = 0;
    if (nnz == 0) return OEM_OK;
    DevBuf<uint64_t> d_idx;
    DevBuf<float> d_f;
    DevBuf<unsigned long long> d_count;
    OEM_TRY(dev_alloc(&d_idx.p, nnz, nullptr));
    OEM_TRY(dev_alloc(&d_f.p, nnz, nullptr));
    OEM_TRY(dev_alloc(&d_count.p, 1, nullptr));
    OEM_HIP(hipMemsetAsync(d_count.p, 0, sizeof(unsigned long long), nullptr));
    hipLaunchKernelGGL(k_proj_collect, dim3((uint32_t)((nnz + kFT - 1) / kFT)), dim3(kFT), 0, nullptr, d_unsure, d_as_prob, nnz, d_count.p,
                       d_idx.p, d_f.p);
    OEM_HIP(hipGetLastError());
    unsigned long long m = 0;
    OEM_HIP(hipMemcpy(&m, d_count.p, sizeof m, hipMemcpyDeviceToHost)); // (the pass's one wait after emit)
    if (m > nnz) return fail(OEM_ERR_STATE, "k_proj_collect: %llu entries for %llu alignments", m, (unsigned long long)nnz);
    if (m == 0) return OEM_OK;
    OEM_TRY(dev_alloc(&d->idx.p, m, nullptr));
    OEM_TRY(dev_alloc(&d->f.p, m, nullptr));
    OEM_HIP(hipMemcpy(d->idx.p, d_idx.p, sizeof(uint64_t) * m, hipMemcpyDeviceToDevice));
    OEM_HIP(hipMemcpy(d->f.p, d_f.p, sizeof(float) * m, hipMemcpyDeviceToDevice));
    d->n = m;
    return OEM_OK;
}

// The alignments k_proj_emit left unsure: their f comes down, libm's expf goes back up.  Segments keep hipcub's int counts.
int finish_on_host(float *d_as_prob, const uint8_t *d_unsure, uint64_t nnz, uint64_t *n_finished)
{
    constexpr uint64_t kSeg = 1ull << 30;
    hipStream_t st = nullptr;
    *n_finished = 0;
    if (nnz == 0) return OEM_OK;
    const uint64_t cap = nnz < kSeg ? nnz : kSeg;
    DevBuf<uint64_t> d_idx;
    DevBuf<float> d_f;
    DevBuf<uint64_t> d_num;
    DevBuf<uint8_t> d_tmp;
    OEM_TRY(dev_alloc(&d_idx.p, cap, nullptr));
    OEM_TRY(dev_alloc(&d_f.p, cap, nullptr));
    OEM_TRY(dev_alloc(&d_num.p, 1, nullptr));
    size_t tmp_i = 0, tmp_f = 0;
    {
        hipcub::CountingInputIterator<uint64_t> in_i(0);
        OEM_HIP(hipcub::DeviceSelect::Flagged(nullptr, tmp_i, in_i, d_unsure, d_idx.p, d_num.p, (int)cap, st));
        OEM_HIP(hipcub::DeviceSelect::Flagged(nullptr, tmp_f, (const float *)d_as_prob, d_unsure, d_f.p, d_num.p, (int)cap, st));
    }
    OEM_TRY(dev_alloc(&d_tmp.p, tmp_i > tmp_f ? tmp_i : tmp_f, nullptr));
    std::vector<float> h_f;
    for (uint64_t s0 = 0; s0 < nnz; s0 += kSeg) {
        const uint64_t n = nnz - s0 < kSeg ? nnz - s0 : kSeg;
        hipcub::CountingInputIterator<uint64_t> in_i(s0);
        OEM_HIP(hipcub::DeviceSelect::Flagged(d_tmp.p, tmp_i, in_i, d_unsure + s0, d_idx.p, d_num.p, (int)n, st));
        OEM_HIP(hipcub::DeviceSelect::Flagged(d_tmp.p, tmp_f, (const float *)d_as_prob + s0, d_unsure + s0, d_f.p, d_num.p, (int)n, st));
        uint64_t m = 0;
        OEM_HIP(hipMemcpy(&m, d_num.p, sizeof(m), hipMemcpyDeviceToHost));
        if (m == 0) continue;
        h_f.resize(m);
        OEM_HIP(hipMemcpy(h_f.data(), d_f.p, sizeof(float) * m, hipMemcpyDeviceToHost));
        for (float &f : h_f) f = expf(f);                                                  // f.exp() (:1282), libm's
        OEM_HIP(hipMemcpy(d_f.p, h_f.data(), sizeof(float) * m, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_proj_scatter, dim3((uint32_t)((m + kFT - 1) / kFT)), dim3(kFT), 0, st, d_idx.p, d_f.p, m, d_as_prob);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipStreamSynchronize(st));
        *n_finished += m;
    }
    return OEM_OK;
}

} // namespace

// Measure, scans, emit and finish of one batch on the current device (oem_filter_device.h).
int proj_device(const char *who, const oem_filters &F, const oem_proj_opts &P, const uint64_t *txp_len, uint32_t n_txps,
                const std::vector<float> &tab, const oem_proj_record *records, const uint64_t *group_off, const uint64_t *read_len,
                uint64_t n_groups, uint64_t base, bool want_coords, bool narrow, FilterResult *out, ProjDeferred *deferred,
                bool pinned_src)
{
    const bool timing = knob("OEM_FILTER_TIMING", 0) != 0;
    const bool by_table = P.prob_source == OEM_PROJ_SCORE;
    const uint64_t n_records = group_off[n_groups];
    const uint64_t chunk = (uint64_t)filter_chunk_groups();

    DevBuf<oem_proj_record> d_recs;
    DevBuf<unsigned long long> d_goff;
    DevBuf<uint64_t> d_read_len, d_aln_off, d_row_idx;
    DevBuf<double> d_best_sim;
    DevBuf<int32_t> d_best_score;
    DevBuf<FilterTotals> d_tot;
    DevBuf<float> d_tab;
    DevBuf<uint8_t> d_unsure;
    OEM_TRY(dev_alloc(&d_recs.p, n_records, nullptr));
    OEM_TRY(dev_alloc(&d_goff.p, n_groups + 1, nullptr));
    OEM_TRY(dev_alloc(&d_read_len.p, n_groups, nullptr));
    OEM_TRY(dev_alloc(&out->n_kept.p, n_groups + 1, nullptr));
    OEM_TRY(dev_alloc(&d_best_sim.p, n_groups, nullptr));
    OEM_TRY(dev_alloc(&d_best_score.p, n_groups, nullptr));
    OEM_TRY(dev_alloc(&d_tot.p, 1, nullptr));
    OEM_TRY(dev_alloc(&out->txp_len.p, n_txps, nullptr));
    FilterTotals h_tot;
    std::memset(&h_tot, 0, sizeof(h_tot));
    h_tot.bad_record = kNoRecord;
    OEM_HIP(hipMemcpy(d_tot.p, &h_tot, sizeof(h_tot), hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_goff.p, group_off, sizeof(uint64_t) * (n_groups + 1), hipMemcpyHostToDevice));
    if (n_groups) OEM_HIP(hipMemcpy(d_read_len.p, read_len, sizeof(uint64_t) * n_groups, hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(out->txp_len.p, txp_len, sizeof(uint64_t) * n_txps, hipMemcpyHostToDevice));
    OEM_HIP(hipMemset(out->n_kept.p + n_groups, 0, sizeof(uint32_t))); // (the scans read n_groups + 1 entries)
    OEM_HIP(hipStreamSynchronize(nullptr)); // (the upload lanes do not wait for the null stream)

    float ms[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    OEM_TRY(filter_upload_measure(records, d_recs.p, group_off, n_groups, chunk, timing ? ms : nullptr,
                                  [&](hipStream_t st, uint64_t g0, uint64_t g1) {
                                      hipLaunchKernelGGL(k_proj_measure, dim3((uint32_t)((g1 - g0 + kFT - 1) / kFT)), dim3(kFT), 0, st,
                                                         F, d_recs.p, d_goff.p, d_read_len.p, g0, g1, out->txp_len.p, n_txps,
                                                         out->n_kept.p, d_best_sim.p, d_best_score.p, d_tot.p);
                                  },
                                  pinned_src));
    g_proj_pass[0] = ms[1];
    OEM_HIP(hipMemcpy(&h_tot, d_tot.p, sizeof(h_tot), hipMemcpyDeviceToHost));
    if (h_tot.flags & kFilterFlagBadRef) {
        const uint32_t ref = records[h_tot.bad_record].ref_id;
        return fail(OEM_ERR_ARG, "%s: record %llu: ref_id %u %s", who, h_tot.bad_record, ref,
                    ref >= n_txps ? "is not below n_txps" : "names a transcript of length 0");
    }
    if (h_tot.flags & kFilterFlagBigScore) {
        out->host_rerun = true;
        return OEM_OK;
    }
    const uint64_t *cnt = (const uint64_t *)h_tot.counts;
    out->dt = oem_discard_table{cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], cnt[5], cnt[6], cnt[7], cnt[8], cnt[9]};

    hipStream_t st = nullptr; // scans, emit and finish follow one another on the null stream (the lanes are idle)
    Event ev[2];
    if (timing)
        for (auto &e : ev) OEM_HIP(hipEventCreate(&e.e));
    OEM_TRY(filter_scan_alloc(who, n_groups, base, want_coords, narrow, out, &d_aln_off, &d_row_idx, nullptr, nullptr));
    const uint64_t nnz = out->nnz;
    if (by_table) {
        OEM_TRY(dev_alloc(&d_tab.p, tab.size(), nullptr));
        if (!tab.empty()) OEM_HIP(hipMemcpy(d_tab.p, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    } else {
        OEM_TRY(dev_alloc(&d_unsure.p, nnz, nullptr));
    }
    if (timing) OEM_HIP(hipEventRecord(ev[0].e, st));
    if (n_groups && nnz) {
        hipLaunchKernelGGL(k_proj_emit, dim3((uint32_t)((n_groups + kFT - 1) / kFT)), dim3(kFT), 0, st, F, P, d_recs.p, d_goff.p,
                           n_groups, out->txp_len.p, n_txps, out->n_kept.p, d_best_sim.p, d_best_score.p, d_aln_off.p,
                           d_row_idx.p, d_tab.p, (uint64_t)tab.size(), base, out->row_ptr64.p, out->row_ptr32.p, out->tid.p,
                           out->as_prob.p, d_unsure.p, out->start.p, out->end.p, out->strand.p);
        OEM_HIP(hipGetLastError());
    }
    if (timing) OEM_HIP(hipEventRecord(ev[1].e, st));
    if (deferred && !by_table) OEM_TRY(collect_deferred(out->as_prob.p, d_unsure.p, nnz, deferred)); // (behind emit on the null stream)
    OEM_HIP(hipStreamSynchronize(st));
    if (timing) {
        float emit_ms = 0.f;
        OEM_HIP(hipEventElapsedTime(&emit_ms, ev[0].e, ev[1].e));
        g_proj_pass[1] = emit_ms;
    }
    d_recs.reset();
    uint64_t n_finished = 0;
    if (!by_table && !deferred) {
        const auto t0 = std::chrono::steady_clock::now();
        OEM_TRY(finish_on_host(out->as_prob.p, d_unsure.p, nnz, &n_finished));
        g_proj_pass[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    g_proj_pass[3] = (double)n_finished;
    g_proj_pass[4] = (double)nnz;
    return OEM_OK;
}

// Whether the host loop has to take the batch from the start: no table for OEM_PROJ_SCORE (score_prob_denom), a beta that
// is not finite for the two sources that use it.
bool proj_host_only(const oem_filters &F, const oem_proj_opts &P, std::vector<float> *tab)
{
    if (P.prob_source == OEM_PROJ_SCORE) return !filter_prob_table(F.score_prob_denom, *tab);
    return !std::isfinite(P.beta);
}

int proj_finish_deferred(const uint64_t *d_idx, float *d_f, uint64_t n, float *d_as_prob)
{
    if (n == 0) return OEM_OK;
    if (n > 0x7fffffffull * kFT) return fail(OEM_ERR_ARG, "proj_finish_deferred: %llu alignments", (unsigned long long)n);
    std::vector<float> h_f(n);
    OEM_HIP(hipMemcpy(h_f.data(), d_f, sizeof(float) * n, hipMemcpyDeviceToHost));
    for (float &f : h_f) f = expf(f);                                                      // f.exp() (:1282), libm's
    OEM_HIP(hipMemcpy(d_f, h_f.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_proj_scatter, dim3((uint32_t)((n + kFT - 1) / kFT)), dim3(kFT), 0, nullptr, d_idx, (const float *)d_f, n, d_as_prob);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipStreamSynchronize(nullptr));
    return OEM_OK;
}

void proj_last_pass(double *out5) { std::memcpy(out5, g_proj_pass, sizeof g_proj_pass); }

} // namespace oem

using namespace oem;

extern "C" int oem_builder_add_projected_groups_device(oem_builder *b, const oem_proj_record *records,
                                                       const uint64_t *group_off, const uint64_t *read_len, uint64_t n_groups,
                                                       const oem_proj_opts *popts, int device, uint32_t *out_kept)
{
    OEM_API_BEGIN
    const char *who = "oem_builder_add_projected_groups_device";
    for (double &v : g_proj_pass) v = 0.;
    if (!b) return fail(OEM_ERR_ARG, "%s: builder is NULL", who);
    OEM_TRY(check_projected_batch(who, records, group_off, read_len, n_groups, popts));
    if (n_groups >= 0x7fffffffull) return fail(OEM_ERR_ARG, "%s: at most 2^31 - 2 groups per call", who);
    std::vector<float> tab;
    const bool host_only = proj_host_only(b->f, *popts, &tab);
    OEM_TRY(ensure_device(device));
    if (host_only) return add_projected_groups_host(b, records, group_off, read_len, n_groups, *popts, out_kept, who);
    FilterResult r;
    OEM_TRY(proj_device(who, b->f, *popts, b->txp_len.data(), (uint32_t)b->txp_len.size(), tab, records, group_off, read_len,
                        n_groups, b->tid.size(), true, false, &r));
    if (r.host_rerun) return add_projected_groups_host(b, records, group_off, read_len, n_groups, *popts, out_kept, who);
    return filter_result_to_builder(b, r, n_groups, out_kept);
    OEM_API_END("oem_builder_add_projected_groups_device")
}

extern "C" int oem_store_create_projected_records(const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                                                  const oem_proj_record *records, const uint64_t *group_off,
                                                  const uint64_t *read_len, uint64_t n_groups, const oem_proj_opts *popts,
                                                  uint32_t bin_width, int model, double growth_rate, int device,
                                                  const oem_store_opts *opts, uint32_t *out_kept,
                                                  oem_discard_table *out_discard, oem_store **out)
{
    OEM_API_BEGIN
    const char *who = "oem_store_create_projected_records";
    for (double &v : g_proj_pass) v = 0.;
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    OEM_TRY(check_store_from_records(who, filters, txp_len, n_txps, bin_width, model, opts));
    OEM_TRY(check_projected_batch(who, records, group_off, read_len, n_groups, popts));
    if (n_groups >= 0x7fffffffull) return fail(OEM_ERR_ARG, "%s: at most 2^31 - 2 groups per call", who);
    std::vector<float> tab;
    const bool host_only = proj_host_only(*filters, *popts, &tab);
    OEM_TRY(ensure_device(device));

    FilterResult r;
    if (!host_only)
        OEM_TRY(proj_device(who, *filters, *popts, txp_len, n_txps, tab, records, group_off, read_len, n_groups, 0, model >= 0,
                            true, &r));
    if (host_only || r.host_rerun) { // the host loop takes the batch: the long way round, same store
        oem_builder hb;
        hb.f = *filters;
        hb.txp_len.assign(txp_len, txp_len + n_txps);
        OEM_TRY(add_projected_groups_host(&hb, records, group_off, read_len, n_groups, *popts, out_kept, who));
        if (hb.tid.size() >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: a resident store needs fewer than 2^32 alignments", who);
        if (out_discard) *out_discard = hb.dt;
        if (model < 0) return oem_builder_store_create(&hb, nullptr, device, opts, out);
        return oem_builder_store_create_coverage(&hb, bin_width, model, growth_rate, device, opts, nullptr, out);
    }
    return filter_result_to_store(who, r, n_txps, n_groups, bin_width, model, growth_rate, device, opts, out_kept, out_discard, out);
    OEM_API_END("oem_store_create_projected_records")
}
