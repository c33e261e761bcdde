// oem_coverage_cells.hip -- the coverage model of every cell of a single-cell run in one call (single_cell.rs:132-137:
// each cell bins only its own retained alignments, runs binomial_continuous_prob on them and normalises its own
// store).  The result equals oem_coverage_probs_device on each cell's slice, concatenated; the arithmetic is the
// same (oem_coverage_common.h) and only the order of the f64 atomic sums differs.
//
// Cells are processed in chunks of consecutive cells that fit a device-memory budget.  Per chunk:
//
//   k_cc_mark        one lane per alignment: its cell (binary search of the chunk's alignment offsets) and the key
//                    cell * T + tid; flags the key in a dense [cells x T] slot table
//   (hipcub scan)    slot table -> segment number of every (cell, transcript) pair that occurs
//   k_cc_segments    one lane per slot: the segment's transcript, cell and number of bins
//   (hipcub scan)    bins per segment -> bin offsets: bins are allocated for the segments only
//   k_cc_bins        one lane per alignment: key -> segment id (kept for the read pass), overlap fractions added into
//                    the segment's bins with f64 atomics, total_weight counted
//   k_cc_bin_probs   one lane per segment: min coverage, f32 counts, logistic or binomial probabilities (the f32
//                    sums and the running max are sequential in the reference, so they stay sequential here)
//   k_cc_reads       one lane per read: per-alignment coverage probability through the segment id, normalised
//
// The dense slot table is chosen over a radix sort of (cell, tid) keys: its size is cells x T words, which on a
// typical chunk (hundreds of thousands of alignments per cell over tens of thousands of transcripts) is several
// times smaller than the nnz 64-bit keys and values a sort would move, and it needs one scan, not eight digit passes.
#include <algorithm>
#include <climits>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "oem_coverage_common.h"
#include "oem_driver.h"

namespace oem {
namespace {

constexpr int kCC = 256;

__global__ __launch_bounds__(kCC) void k_cc_mark(const uint32_t *__restrict__ tid, const uint32_t *__restrict__ cell_aln_off,
                                                 uint32_t n_cells, uint32_t n_txps, uint32_t nnz,
                                                 uint32_t *__restrict__ key, uint32_t *__restrict__ flag)
{
    const uint64_t j64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; // nnz may be up to 2^32 - 1
    if (j64 >= nnz) return;
    const uint32_t j = (uint32_t)j64;
    uint32_t lo = 0, hi = n_cells; // the last cell c with cell_aln_off[c] <= j (empty cells share offsets)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cell_aln_off[mid] <= j) lo = mid; else hi = mid;
    }
    const uint32_t k = lo * n_txps + tid[j];
    key[j] = k;
    flag[k] = 1u;
}

__global__ __launch_bounds__(kCC) void k_cc_segments(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                     uint32_t n_slots, uint32_t n_txps, const uint32_t *__restrict__ n_bins,
                                                     uint32_t *__restrict__ seg_tid, uint32_t *__restrict__ seg_cell,
                                                     unsigned long long *__restrict__ seg_nb)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_slots || !flag[k]) return;
    const uint32_t s = pos[k], t = k % n_txps;
    seg_tid[s] = t;
    seg_cell[s] = k / n_txps;
    seg_nb[s] = n_bins[t];
}

__global__ __launch_bounds__(kCC) void k_cc_bins(uint32_t *__restrict__ key_seg, const uint32_t *__restrict__ pos,
                                                 const uint32_t *__restrict__ tid, const uint32_t *__restrict__ aln_start,
                                                 const uint32_t *__restrict__ aln_end, const uint64_t *__restrict__ txp_len,
                                                 const uint32_t *__restrict__ n_bins, const unsigned long long *__restrict__ seg_off,
                                                 const uint32_t *__restrict__ seg_cell, uint32_t nnz, double *__restrict__ bins,
                                                 uint32_t *__restrict__ total_weight, uint32_t *__restrict__ err)
{
    const uint64_t j64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j64 >= nnz) return;
    const uint32_t j = (uint32_t)j64;
    const uint32_t s = pos[key_seg[j]];
    key_seg[j] = s; // the read pass looks the alignment's bins up through its segment
    const uint32_t t = tid[j];
    if (!cov_add_interval(aln_start[j], aln_end[j], n_bins[t], (double)txp_len[t], bins + seg_off[s], err + seg_cell[s]))
        return;
    atomicAdd(&total_weight[s], 1u);                                               // :537 (weight 1.0, :727)
}

__global__ __launch_bounds__(kCC) void k_cc_bin_probs(const uint64_t *__restrict__ txp_len, const uint32_t *__restrict__ seg_tid,
                                                      const uint32_t *__restrict__ seg_cell,
                                                      const unsigned long long *__restrict__ seg_off,
                                                      const uint32_t *__restrict__ total_weight, uint32_t n_segs, int model,
                                                      double growth_rate, double *__restrict__ bins, double *__restrict__ prob,
                                                      uint32_t *__restrict__ err)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_segs) return;
    const unsigned long long o = seg_off[s];
    cov_bin_probs(bins + o, prob + o, (uint32_t)(seg_off[s + 1] - o), (double)txp_len[seg_tid[s]], total_weight[s], model,
                  growth_rate, err + seg_cell[s]);
}

__global__ __launch_bounds__(kCC) void k_cc_reads(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ seg,
                                                  const uint32_t *__restrict__ tid, const uint32_t *__restrict__ aln_start,
                                                  const uint32_t *__restrict__ aln_end, const uint64_t *__restrict__ txp_len,
                                                  const uint32_t *__restrict__ n_bins, const unsigned long long *__restrict__ seg_off,
                                                  const uint32_t *__restrict__ seg_cell, const double *__restrict__ prob,
                                                  uint32_t n_reads, double bin_length, double *__restrict__ out,
                                                  uint32_t *__restrict__ err)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t b = row_ptr[r], e = row_ptr[r + 1];
    if (b == e) return;
    cov_normalize_read(b, e, aln_start, aln_end, bin_length,
                       [&](uint64_t j) {
                           const uint32_t t = tid[j];
                           return CovTxpBins{prob + seg_off[seg[j]], n_bins[t], (double)txp_len[t]};
                       },
                       out, err + seg_cell[seg[b]]);
}

// The checks oem_coverage_probs_device makes on every transcript of the annotation, touched or not: they fail any
// cell that has alignments.
__global__ __launch_bounds__(kCC) void k_cc_txp_check(const uint64_t *__restrict__ txp_len, const uint32_t *__restrict__ n_bins,
                                                      uint32_t n_txps, uint32_t *__restrict__ err)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_txps) return;
    const uint32_t n = n_bins[t];
    if (n == 0) { atomicOr(err, kCovErrNoBins); return; }
    const double lenf = (double)txp_len[t];
    const float bwf = (float)round(lenf / (double)n), lenf32 = (float)lenf;        // as cov_bin_probs
    for (uint32_t i = 0; i < n; ++i) {
        const float bs = (float)i * bwf, be = fminf(((float)i + 1.0f) * bwf, lenf32);
        if (!(be > bs)) { atomicOr(err, kCovErrDegenerate); return; }
    }
}

__global__ void k_cc_bin_counts(const uint64_t *__restrict__ txp_len, uint32_t n_txps, uint32_t bin_width,
                                uint32_t *__restrict__ n_bins)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_txps) n_bins[t] = cov_n_bins(txp_len[t], bin_width);
}

const char *cov_err_text(uint32_t f)
{
    if (f & kCovErrInterval) return "add_interval: an alignment lies outside its transcript";
    if (f & kCovErrOlfrac) return "coverage computation error: overlap fraction above 1";
    if (f & kCovErrNoBins) return "a transcript has no coverage bins";
    if (f & kCovErrDegenerate) return "degenerate coverage bin (assert, oarfish_types.rs:490)";
    return "coverage model: non-finite probability";
}

// Device buffers of one call, grown on demand and released at the end.
struct Arena {
    std::vector<void *> p;
    template <typename T> int get(T **q, size_t n)
    {
        *q = nullptr;
        OEM_HIP(hipMalloc((void **)q, (n ? n : 1) * sizeof(T)));
        p.push_back(*q);
        return OEM_OK;
    }
    template <typename T> int grow(T **q, size_t *cap, size_t n)
    {
        if (*q && n <= *cap) return OEM_OK;
        if (*q) {
            p.erase(std::find(p.begin(), p.end(), (void *)*q));
            OEM_HIP(hipFree(*q));
        }
        *cap = std::max(n, (size_t)1);
        return get(q, *cap);
    }
    ~Arena() { for (void *q : p) (void)hipFree(q); }
};

struct Chunk {
    uint32_t c0, c1;     // cells [c0, c1)
    uint64_t r0, r1;     // reads
    uint64_t a0, a1;     // alignments
};

} // namespace
} // namespace oem

using namespace oem;

extern "C" int oem_coverage_probs_cells_device(const uint64_t *cell_row_off, uint32_t n_cells, const uint64_t *row_ptr,
                                               const uint32_t *tid, const uint32_t *aln_start, const uint32_t *aln_end,
                                               const uint64_t *txp_len, uint64_t n_reads, uint64_t nnz, uint32_t n_txps,
                                               uint32_t bin_width, int model, double growth_rate, int device,
                                               double *out_cov_prob)
{
    OEM_API_BEGIN
    const char *who = "oem_coverage_probs_cells_device";
    if (!cell_row_off || !row_ptr || !txp_len || (nnz && (!tid || !aln_start || !aln_end || !out_cov_prob)))
        return fail(OEM_ERR_ARG, "%s: NULL argument", who);
    if (bin_width == 0)
        return fail(OEM_ERR_ARG, "coverage model with 0 bin width is not implemented (logistic_probability.rs:59, binomial_probability.rs:192)");
    if (model != 0 && model != 1) return fail(OEM_ERR_ARG, "%s: model must be 0 (logistic) or 1 (binomial)", who);
    if (n_txps == 0) return fail(OEM_ERR_ARG, "%s: n_txps is 0", who);
    if (n_txps >= (uint32_t)INT_MAX) return fail(OEM_ERR_ARG, "%s: needs n_txps < 2^31 - 1", who);
    if (nnz >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: needs nnz < 2^32", who);
    if (n_reads >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: needs n_reads < 2^32", who);
    if (cell_row_off[0] != 0 || cell_row_off[n_cells] != n_reads)
        return fail(OEM_ERR_ARG, "%s: cell_row_off must span [0, n_reads]", who);
    for (uint32_t c = 0; c < n_cells; ++c)
        if (cell_row_off[c + 1] < cell_row_off[c])
            return fail(OEM_ERR_ARG, "%s: cell_row_off not non-decreasing at cell %u", who, c);
    StageTimer tm;
    OEM_TRY(validate_csr(row_ptr, tid, n_reads, nnz, n_txps));
    tm.lap("cov cells: range checks");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device < 0 || device >= n_dev)
        return fail(OEM_ERR_NO_DEVICE, "%s: no HIP device %d", who, device);
    OEM_HIP(hipSetDevice(device));
    if (nnz == 0) return OEM_OK;

    // ---- chunks of consecutive cells.  A cell's bins are bounded by every transcript's bins and by one new
    // segment of the widest transcript per alignment; its other buffers are known from its size.
    std::vector<uint32_t> h_nb(n_txps);
    uint64_t all_bins = 0, max_nb = 0;
    for (uint32_t t = 0; t < n_txps; ++t) {
        h_nb[t] = cov_n_bins(txp_len[t], bin_width);
        all_bins += h_nb[t];
        max_nb = std::max<uint64_t>(max_nb, h_nb[t]);
    }
    size_t free_b = 0, total_b = 0;
    OEM_HIP(hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget_bytes = free_b / 2;
    const uint64_t budget_bins = (uint64_t)knob("OEM_COV_CELLS_CHUNK_BINS", 0); // testing build: force small chunks
    std::vector<Chunk> chunks;
    {
        Chunk ch{0, 0, 0, 0, 0, 0};
        uint64_t bins = 0, bytes = 0;
        for (uint32_t c = 0; c < n_cells; ++c) {
            const uint64_t reads = cell_row_off[c + 1] - cell_row_off[c];
            const uint64_t a = row_ptr[cell_row_off[c + 1]] - row_ptr[cell_row_off[c]];
            const uint64_t ub = std::min(all_bins, a * max_nb);
            const uint64_t by = 16 * ub + 8 * (uint64_t)n_txps + 28 * std::min<uint64_t>(a, n_txps) + 24 * a + 4 * reads + 8;
            const bool full = ch.c1 > ch.c0 &&
                              (bytes + by > budget_bytes || (budget_bins && bins + ub > budget_bins) ||
                               (uint64_t)(ch.c1 - ch.c0 + 1) * n_txps + 1 > (uint64_t)INT_MAX);
            if (full) {
                chunks.push_back(ch);
                ch = Chunk{c, c, ch.r1, ch.r1, ch.a1, ch.a1};
                bins = bytes = 0;
            }
            ch.c1 = c + 1;
            ch.r1 += reads;
            ch.a1 += a;
            bins += ub;
            bytes += by;
        }
        if (ch.c1 > ch.c0) chunks.push_back(ch);
    }
    uint64_t max_cells = 0, max_reads = 0, max_aln = 0;
    for (const Chunk &ch : chunks) {
        max_cells = std::max<uint64_t>(max_cells, ch.c1 - ch.c0);
        max_reads = std::max(max_reads, ch.r1 - ch.r0);
        max_aln = std::max(max_aln, ch.a1 - ch.a0);
    }
    const uint64_t max_slots = max_cells * n_txps + 1;
    const uint64_t max_segs = std::min<uint64_t>(max_slots - 1, max_aln) + 1;
    tm.lap("cov cells: plan");

    hipStream_t st = nullptr;
    OEM_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard {
        hipStream_t s;
        ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    } sg{st};
    Arena ar;
    uint32_t *d_nb, *d_tid, *d_start, *d_end, *d_key, *d_rp, *d_coff, *d_flag, *d_pos, *d_seg_tid, *d_seg_cell, *d_tw, *d_err,
        *d_gerr;
    uint64_t *d_len;
    unsigned long long *d_seg_nb, *d_seg_off;
    double *d_out, *d_bins = nullptr, *d_prob = nullptr;
    size_t cap_bins = 0, cap_prob = 0;
    OEM_TRY(ar.get(&d_len, n_txps));
    OEM_TRY(ar.get(&d_nb, n_txps));
    OEM_TRY(ar.get(&d_gerr, 1));
    OEM_TRY(ar.get(&d_tid, max_aln));
    OEM_TRY(ar.get(&d_start, max_aln));
    OEM_TRY(ar.get(&d_end, max_aln));
    OEM_TRY(ar.get(&d_key, max_aln));
    OEM_TRY(ar.get(&d_out, max_aln));
    OEM_TRY(ar.get(&d_rp, max_reads + 1));
    OEM_TRY(ar.get(&d_coff, max_cells + 1));
    OEM_TRY(ar.get(&d_err, max_cells));
    OEM_TRY(ar.get(&d_flag, max_slots));
    OEM_TRY(ar.get(&d_pos, max_slots));
    OEM_TRY(ar.get(&d_seg_tid, max_segs));
    OEM_TRY(ar.get(&d_seg_cell, max_segs));
    OEM_TRY(ar.get(&d_tw, max_segs));
    OEM_TRY(ar.get(&d_seg_nb, max_segs));
    OEM_TRY(ar.get(&d_seg_off, max_segs));
    size_t tmp_bytes = 0, tmp2 = 0;
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_flag, d_pos, (int)max_slots, st));
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, d_seg_nb, d_seg_off, (int)max_segs, st));
    void *d_tmp;
    OEM_TRY(ar.get((char **)&d_tmp, std::max(tmp_bytes, tmp2)));
    tmp_bytes = std::max(tmp_bytes, tmp2);

    OEM_HIP(hipMemcpyAsync(d_len, txp_len, sizeof(uint64_t) * n_txps, hipMemcpyHostToDevice, st));
    OEM_HIP(hipMemsetAsync(d_gerr, 0, sizeof(uint32_t), st));
    const uint32_t tg = (n_txps + kCC - 1) / kCC;
    hipLaunchKernelGGL(k_cc_bin_counts, dim3(tg), dim3(kCC), 0, st, d_len, n_txps, bin_width, d_nb);
    hipLaunchKernelGGL(k_cc_txp_check, dim3(tg), dim3(kCC), 0, st, d_len, d_nb, n_txps, d_gerr);
    OEM_HIP(hipGetLastError());
    uint32_t h_gerr = 0;
    OEM_HIP(hipMemcpyAsync(&h_gerr, d_gerr, sizeof(uint32_t), hipMemcpyDeviceToHost, st));

    std::vector<uint32_t> h_rp(max_reads + 1), h_coff(max_cells + 1), h_err(max_cells);
    for (const Chunk &ch : chunks) {
        const uint32_t ncc = ch.c1 - ch.c0;
        const uint32_t nr = (uint32_t)(ch.r1 - ch.r0), na = (uint32_t)(ch.a1 - ch.a0);
        const uint32_t n_slots = ncc * n_txps;
        for (uint32_t c = 0; c <= ncc; ++c) h_coff[c] = (uint32_t)(row_ptr[cell_row_off[ch.c0 + c]] - ch.a0);
        for (uint64_t r = 0; r <= nr; ++r) h_rp[r] = (uint32_t)(row_ptr[ch.r0 + r] - ch.a0);
        OEM_HIP(hipMemcpyAsync(d_coff, h_coff.data(), sizeof(uint32_t) * (ncc + 1), hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(d_rp, h_rp.data(), sizeof(uint32_t) * ((size_t)nr + 1), hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(d_tid, tid + ch.a0, sizeof(uint32_t) * (size_t)na, hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(d_start, aln_start + ch.a0, sizeof(uint32_t) * (size_t)na, hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(d_end, aln_end + ch.a0, sizeof(uint32_t) * (size_t)na, hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemsetAsync(d_flag, 0, sizeof(uint32_t) * ((size_t)n_slots + 1), st));
        OEM_HIP(hipMemsetAsync(d_err, 0, sizeof(uint32_t) * ncc, st));
        const dim3 ag((uint32_t)(((uint64_t)na + kCC - 1) / kCC));
        if (na) hipLaunchKernelGGL(k_cc_mark, ag, dim3(kCC), 0, st, d_tid, d_coff, ncc, n_txps, na, d_key, d_flag);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_flag, d_pos, (int)n_slots + 1, st));
        uint32_t n_segs = 0;
        OEM_HIP(hipMemcpyAsync(&n_segs, d_pos + n_slots, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        OEM_HIP(hipStreamSynchronize(st));
        if (n_segs == 0) continue; // the chunk's cells have no alignments
        hipLaunchKernelGGL(k_cc_segments, dim3((n_slots + kCC - 1) / kCC), dim3(kCC), 0, st, d_flag, d_pos, n_slots, n_txps,
                           d_nb, d_seg_tid, d_seg_cell, d_seg_nb);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemsetAsync(d_seg_nb + n_segs, 0, sizeof(unsigned long long), st));
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_seg_nb, d_seg_off, (int)n_segs + 1, st));
        unsigned long long n_bins = 0;
        OEM_HIP(hipMemcpyAsync(&n_bins, d_seg_off + n_segs, sizeof(n_bins), hipMemcpyDeviceToHost, st));
        OEM_HIP(hipStreamSynchronize(st));
        OEM_TRY(ar.grow(&d_bins, &cap_bins, n_bins));
        OEM_TRY(ar.grow(&d_prob, &cap_prob, n_bins));
        OEM_HIP(hipMemsetAsync(d_bins, 0, sizeof(double) * (n_bins ? n_bins : 1), st));
        OEM_HIP(hipMemsetAsync(d_tw, 0, sizeof(uint32_t) * n_segs, st));
        hipLaunchKernelGGL(k_cc_bins, ag, dim3(kCC), 0, st, d_key, d_pos, d_tid, d_start, d_end, d_len, d_nb, d_seg_off,
                           d_seg_cell, na, d_bins, d_tw, d_err);
        hipLaunchKernelGGL(k_cc_bin_probs, dim3((n_segs + kCC - 1) / kCC), dim3(kCC), 0, st, d_len, d_seg_tid, d_seg_cell,
                           d_seg_off, d_tw, n_segs, model, growth_rate, d_bins, d_prob, d_err);
        if (nr)
            hipLaunchKernelGGL(k_cc_reads, dim3((uint32_t)(((uint64_t)nr + kCC - 1) / kCC)), dim3(kCC), 0, st, d_rp, d_key, d_tid, d_start, d_end,
                               d_len, d_nb, d_seg_off, d_seg_cell, d_prob, nr, (double)bin_width, d_out, d_err);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpyAsync(h_err.data(), d_err, sizeof(uint32_t) * ncc, hipMemcpyDeviceToHost, st));
        OEM_HIP(hipMemcpyAsync(out_cov_prob + ch.a0, d_out, sizeof(double) * (size_t)na, hipMemcpyDeviceToHost, st));
        OEM_HIP(hipStreamSynchronize(st));
        for (uint32_t c = 0; c < ncc; ++c) {
            const bool has_aln = h_coff[c + 1] > h_coff[c];
            const uint32_t f = h_err[c] | (has_aln ? h_gerr : 0u);
            if (f) return fail(OEM_ERR_STATE, "%s: cell %u: %s", who, ch.c0 + c, cov_err_text(f));
        }
    }
    tm.lap("cov cells: chunks");
    return OEM_OK;
    OEM_API_END("oem_coverage_probs_cells_device")
}
