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
// The same chunk body (run_chunk) serves oem_em_run_cells_coverage_sparse (cells_coverage_group): there a group of
// the cells EM uploads its arrays once, runs the chunks over them, and k_cc_weights turns the column into the
// store's f64 weights on the device.
//
// The dense slot table is chosen over a radix sort of (cell, tid) keys: its size is cells x T words, which on a
// typical chunk (hundreds of thousands of alignments per cell over tens of thousands of transcripts) is several
// times smaller than the nnz 64-bit keys and values a sort would move, and it needs one scan, not eight digit passes.
#include <algorithm>
#include <climits>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "oem_cells.h"
#include "oem_coverage_common.h"

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
                                                  uint32_t n_reads, uint32_t aln_base, double bin_length,
                                                  double *__restrict__ out, uint32_t *__restrict__ err)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t b = row_ptr[r] - aln_base, e = row_ptr[r + 1] - aln_base; // (row_ptr: relative to the resident arrays)
    if (b == e) return;
    cov_normalize_read(b, e, aln_start, aln_end, bin_length,
                       [&](uint64_t j) {
                           const uint32_t t = tid[j];
                           return CovTxpBins{prob + seg_off[seg[j]], n_bins[t], (double)txp_len[t]};
                       },
                       out, err + seg_cell[seg[b]]);
}

// em.rs:107-111's iteration-invariant factor w = (p as f64) * cov of every alignment, the expression of upload_csr, so
// the stream is bit-identical to the one a host coverage column gives.  A read with a NaN coverage (the 0/0 of a
// zero-span alignment) gets w = p * 0 on every alignment, as zero_nan_rows leaves it: the EM drops it (em.rs:115).
__global__ __launch_bounds__(kCC) void k_cc_weights(const uint32_t *__restrict__ row_ptr, const float *__restrict__ p,
                                                    const double *__restrict__ cov, uint32_t n_reads,
                                                    double *__restrict__ w)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t b = row_ptr[r], e = row_ptr[r + 1];
    bool nan = false;
    for (uint32_t j = b; j < e; ++j) nan |= cov[j] != cov[j];
    for (uint32_t j = b; j < e; ++j) w[j] = (double)p[j] * (nan ? 0.0 : cov[j]);
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

// Cuts cells [0, n_cells) into chunks of consecutive cells that fit `budget_bytes` (and the testing build's bin
// budget).  A cell's bins are bounded by every transcript's bins and by one new segment of the widest transcript per
// alignment; its other buffers are known from its size (`per_aln`, `per_read`: the bytes a chunk holds for each of its
// alignments and reads besides the slot table, segments and bins).
std::vector<Chunk> plan_chunks(const uint64_t *cell_row_off, uint32_t n_cells, const uint64_t *row_ptr, uint32_t n_txps,
                               uint64_t all_bins, uint64_t max_nb, uint64_t budget_bytes, uint64_t per_aln, uint64_t per_read,
                               const uint64_t *cell_aln_off = nullptr /* given: row_ptr[cell_row_off[c]], row_ptr not read */)
{
    auto aln_at = [&](uint32_t c) { return cell_aln_off ? cell_aln_off[c] : row_ptr[cell_row_off[c]]; };
    const uint64_t budget_bins = (uint64_t)knob("OEM_COV_CELLS_CHUNK_BINS", 0); // testing build: force small chunks
    std::vector<Chunk> chunks;
    Chunk ch{0, 0, cell_row_off[0], cell_row_off[0], aln_at(0), aln_at(0)};
    uint64_t bins = 0, bytes = 0;
    for (uint32_t c = 0; c < n_cells; ++c) {
        const uint64_t reads = cell_row_off[c + 1] - cell_row_off[c];
        const uint64_t a = aln_at(c + 1) - aln_at(c);
        const uint64_t ub = std::min(all_bins, a * max_nb);
        const uint64_t by = 16 * ub + 8 * (uint64_t)n_txps + 28 * std::min<uint64_t>(a, n_txps) + per_aln * a + per_read * reads + 8;
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
    return chunks;
}

// The device buffers of the per-chunk steps, sized for the largest chunk (bins and probabilities grow on demand).
struct ChunkBufs {
    uint32_t *key, *coff, *flag, *pos, *seg_tid, *seg_cell, *tw, *err;
    unsigned long long *seg_nb, *seg_off;
    double *bins = nullptr, *prob = nullptr;
    size_t cap_bins = 0, cap_prob = 0;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
};

int alloc_chunk_bufs(hipStream_t st, Arena &ar, const std::vector<Chunk> &chunks, uint32_t n_txps, ChunkBufs *b)
{
    uint64_t max_cells = 0, max_aln = 0;
    for (const Chunk &ch : chunks) {
        max_cells = std::max<uint64_t>(max_cells, ch.c1 - ch.c0);
        max_aln = std::max(max_aln, ch.a1 - ch.a0);
    }
    const uint64_t max_slots = max_cells * n_txps + 1;
    const uint64_t max_segs = std::min<uint64_t>(max_slots - 1, max_aln) + 1;
    OEM_TRY(ar.get(&b->key, max_aln));
    OEM_TRY(ar.get(&b->coff, max_cells + 1));
    OEM_TRY(ar.get(&b->err, max_cells));
    OEM_TRY(ar.get(&b->flag, max_slots));
    OEM_TRY(ar.get(&b->pos, max_slots));
    OEM_TRY(ar.get(&b->seg_tid, max_segs));
    OEM_TRY(ar.get(&b->seg_cell, max_segs));
    OEM_TRY(ar.get(&b->tw, max_segs));
    OEM_TRY(ar.get(&b->seg_nb, max_segs));
    OEM_TRY(ar.get(&b->seg_off, max_segs));
    size_t t1 = 0, t2 = 0;
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t1, b->flag, b->pos, (int)max_slots, st));
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, b->seg_nb, b->seg_off, (int)max_segs, st));
    b->tmp_bytes = std::max(t1, t2);
    OEM_TRY(ar.get((char **)&b->tmp, b->tmp_bytes));
    return OEM_OK;
}

// The coverage of one chunk of `ncc` cells whose alignments are [0, na) of tid / start / end / out and whose reads are
// [0, nr) of row_ptr (values relative to `aln_base` before it); h_coff: the cells' alignment offsets relative to the
// chunk.  On return h_err[0, ncc) holds every cell's error bits (the annotation-wide ones not included).
int run_chunk(hipStream_t st, Arena &ar, ChunkBufs &b, const uint64_t *d_len, const uint32_t *d_nb, uint32_t n_txps,
              uint32_t bin_width, int model, double growth_rate, uint32_t ncc, uint32_t nr, uint32_t na,
              const uint32_t *h_coff, const uint32_t *d_rp, uint32_t aln_base, const uint32_t *d_tid,
              const uint32_t *d_start, const uint32_t *d_end, double *d_out, uint32_t *h_err)
{
    const uint32_t n_slots = ncc * n_txps;
    OEM_HIP(hipMemcpyAsync(b.coff, h_coff, sizeof(uint32_t) * (ncc + 1), hipMemcpyHostToDevice, st));
    OEM_HIP(hipMemsetAsync(b.flag, 0, sizeof(uint32_t) * ((size_t)n_slots + 1), st));
    OEM_HIP(hipMemsetAsync(b.err, 0, sizeof(uint32_t) * ncc, st));
    const dim3 ag((uint32_t)(((uint64_t)na + kCC - 1) / kCC));
    if (na) hipLaunchKernelGGL(k_cc_mark, ag, dim3(kCC), 0, st, d_tid, b.coff, ncc, n_txps, na, b.key, b.flag);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(b.tmp, b.tmp_bytes, b.flag, b.pos, (int)n_slots + 1, st));
    uint32_t n_segs = 0;
    OEM_HIP(hipMemcpyAsync(&n_segs, b.pos + n_slots, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    OEM_HIP(hipStreamSynchronize(st));
    if (n_segs == 0) { // the chunk's cells have no alignments
        std::fill(h_err, h_err + ncc, 0u);
        return OEM_OK;
    }
    hipLaunchKernelGGL(k_cc_segments, dim3((n_slots + kCC - 1) / kCC), dim3(kCC), 0, st, b.flag, b.pos, n_slots, n_txps,
                       d_nb, b.seg_tid, b.seg_cell, b.seg_nb);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemsetAsync(b.seg_nb + n_segs, 0, sizeof(unsigned long long), st));
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(b.tmp, b.tmp_bytes, b.seg_nb, b.seg_off, (int)n_segs + 1, st));
    unsigned long long n_bins = 0;
    OEM_HIP(hipMemcpyAsync(&n_bins, b.seg_off + n_segs, sizeof(n_bins), hipMemcpyDeviceToHost, st));
    OEM_HIP(hipStreamSynchronize(st));
    OEM_TRY(ar.grow(&b.bins, &b.cap_bins, n_bins));
    OEM_TRY(ar.grow(&b.prob, &b.cap_prob, n_bins));
    OEM_HIP(hipMemsetAsync(b.bins, 0, sizeof(double) * (n_bins ? n_bins : 1), st));
    OEM_HIP(hipMemsetAsync(b.tw, 0, sizeof(uint32_t) * n_segs, st));
    hipLaunchKernelGGL(k_cc_bins, ag, dim3(kCC), 0, st, b.key, b.pos, d_tid, d_start, d_end, d_len, d_nb, b.seg_off,
                       b.seg_cell, na, b.bins, b.tw, b.err);
    hipLaunchKernelGGL(k_cc_bin_probs, dim3((n_segs + kCC - 1) / kCC), dim3(kCC), 0, st, d_len, b.seg_tid, b.seg_cell,
                       b.seg_off, b.tw, n_segs, model, growth_rate, b.bins, b.prob, b.err);
    if (nr)
        hipLaunchKernelGGL(k_cc_reads, dim3((uint32_t)(((uint64_t)nr + kCC - 1) / kCC)), dim3(kCC), 0, st, d_rp, b.key, d_tid,
                           d_start, d_end, d_len, d_nb, b.seg_off, b.seg_cell, b.prob, nr, aln_base, (double)bin_width,
                           d_out, b.err);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpyAsync(h_err, b.err, sizeof(uint32_t) * ncc, hipMemcpyDeviceToHost, st));
    OEM_HIP(hipStreamSynchronize(st));
    return OEM_OK;
}

// txp_len and the per-transcript bin counts on the device, and the checks every transcript must pass
int setup_txps(hipStream_t st, const uint64_t *txp_len, uint32_t n_txps, uint32_t bin_width, uint64_t *d_len,
               uint32_t *d_nb, uint32_t *d_gerr, uint32_t *h_gerr)
{
    OEM_HIP(hipMemcpyAsync(d_len, txp_len, sizeof(uint64_t) * n_txps, hipMemcpyHostToDevice, st));
    OEM_HIP(hipMemsetAsync(d_gerr, 0, sizeof(uint32_t), st));
    const uint32_t tg = (n_txps + kCC - 1) / kCC;
    hipLaunchKernelGGL(k_cc_bin_counts, dim3(tg), dim3(kCC), 0, st, d_len, n_txps, bin_width, d_nb);
    hipLaunchKernelGGL(k_cc_txp_check, dim3(tg), dim3(kCC), 0, st, d_len, d_nb, n_txps, d_gerr);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpyAsync(h_gerr, d_gerr, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return OEM_OK;
}

struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard()
    {
        if (!s) return;
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
};

} // namespace

int cells_coverage_setup(CellsCoverage *cc)
{
    uint64_t all_bins = 0, max_nb = 0;
    for (uint32_t t = 0; t < cc->n_txps; ++t) {
        const uint64_t nb = cov_n_bins(cc->txp_len[t], cc->bin_width);
        all_bins += nb;
        max_nb = std::max(max_nb, nb);
    }
    cc->all_bins = all_bins;
    cc->max_nb = max_nb;
    StreamGuard sg;
    OEM_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    DevBuf<uint32_t> d_gerr;
    OEM_TRY(dev_alloc(&d_gerr.p, 1, nullptr));
    OEM_TRY(dev_alloc(&cc->d_len, cc->n_txps, nullptr));
    OEM_TRY(dev_alloc(&cc->d_nb, cc->n_txps, nullptr));
    OEM_TRY(setup_txps(sg.s, cc->txp_len, cc->n_txps, cc->bin_width, cc->d_len, cc->d_nb, d_gerr.p, &cc->gerr));
    OEM_HIP(hipStreamSynchronize(sg.s));
    return OEM_OK;
}

int check_cells_coverage_args(const char *who, uint32_t bin_width, int model, uint32_t n_txps, uint64_t nnz, uint64_t n_reads)
{
    if (bin_width == 0)
        return fail(OEM_ERR_ARG, "coverage model with 0 bin width is not implemented (logistic_probability.rs:59, binomial_probability.rs:192)");
    if (model != 0 && model != 1) return fail(OEM_ERR_ARG, "%s: model must be 0 (logistic) or 1 (binomial)", who);
    if (n_txps == 0) return fail(OEM_ERR_ARG, "%s: n_txps is 0", who);
    if (n_txps >= (uint32_t)INT_MAX) return fail(OEM_ERR_ARG, "%s: needs n_txps < 2^31 - 1", who);
    if (nnz >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: needs nnz < 2^32", who);
    if (n_reads >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: needs n_reads < 2^32", who);
    return OEM_OK;
}

int cells_coverage_group(const CellsCoverage &cc, const CellsGroup &g, ResidentCsr *out)
{
    StageTimer tm;
    const uint64_t n_reads = g.n_reads, nnz = g.nnz;
    const char *who = "oem_em_run_cells_coverage_sparse";
    StreamGuard sg;
    OEM_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    hipStream_t st = sg.s;
    // 1. what the store keeps (caller order: row pointers narrowed on the device, ids, the weights written below)
    if (!out->row_ptr) {
        OEM_TRY(dev_alloc(&out->row_ptr, n_reads + 1, nullptr));
        OEM_TRY(upload_row_ptr_u32(st, g.row_ptr, n_reads + 1, out->row_ptr));
    }
    const bool on_device = g.d_aln_start != nullptr; // (a group filtered from records: nothing to upload)
    if (!on_device) OEM_TRY(dev_alloc(&out->tid, nnz, nullptr));
    OEM_TRY(dev_alloc(&out->w64, nnz, nullptr));
    if (nnz == 0) return OEM_OK;
    // the coverage scratch: released when this scope ends, before the store's layout is built
    Arena ar;
    const uint32_t *d_start = g.d_aln_start, *d_end = g.d_aln_end;
    const float *d_p = g.d_as_prob;
    double *d_cov;
    OEM_TRY(ar.get(&d_cov, nnz));
    if (!on_device) {
        uint32_t *u_start, *u_end;
        float *u_p;
        OEM_HIP(hipMemcpyAsync(out->tid, g.tid, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice, st));
        OEM_TRY(ar.get(&u_start, nnz));
        OEM_TRY(ar.get(&u_end, nnz));
        OEM_TRY(ar.get(&u_p, nnz));
        OEM_HIP(hipMemcpyAsync(u_start, g.aln_start, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(u_end, g.aln_end, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(u_p, g.as_prob, sizeof(float) * nnz, hipMemcpyHostToDevice, st));
        OEM_HIP(hipStreamSynchronize(st));
        d_start = u_start;
        d_end = u_end;
        d_p = u_p;
        tm.lap("cov+em: group upload");
    }

    // 2. coverage, in sub-chunks of consecutive cells over the resident arrays when the slot tables and bins of all
    // of them do not fit half the free memory
    size_t free_b = 0, total_b = 0;
    OEM_HIP(hipMemGetInfo(&free_b, &total_b));
    const std::vector<Chunk> chunks = plan_chunks(g.cell_row_off, g.n_cells, g.row_ptr, cc.n_txps, cc.all_bins, cc.max_nb,
                                                  free_b / 2, 4 /* segment ids */, 0, g.cell_aln_off);
    ChunkBufs b;
    OEM_TRY(alloc_chunk_bufs(st, ar, chunks, cc.n_txps, &b));
    std::vector<uint32_t> h_coff, h_err;
    for (const Chunk &ch : chunks) {
        const uint32_t ncc = ch.c1 - ch.c0;
        h_coff.resize((size_t)ncc + 1);
        h_err.resize(ncc);
        for (uint32_t c = 0; c <= ncc; ++c) h_coff[c] = (uint32_t)(g.cell_aln_off[ch.c0 + c] - ch.a0);
        OEM_TRY(run_chunk(st, ar, b, cc.d_len, cc.d_nb, cc.n_txps, cc.bin_width, cc.model, cc.growth_rate, ncc,
                          (uint32_t)(ch.r1 - ch.r0), (uint32_t)(ch.a1 - ch.a0), h_coff.data(), out->row_ptr + ch.r0,
                          (uint32_t)ch.a0, out->tid + ch.a0, d_start + ch.a0, d_end + ch.a0, d_cov + ch.a0, h_err.data()));
        for (uint32_t c = 0; c < ncc; ++c) {
            const uint32_t f = h_err[c] | (h_coff[c + 1] > h_coff[c] ? cc.gerr : 0u);
            if (f) return fail(OEM_ERR_STATE, "%s: cell %llu: %s", who, (unsigned long long)(g.first_cell + ch.c0 + c), cov_err_text(f));
        }
    }
    tm.lap("cov+em: coverage");
    // 3. the column the EM uses, for the caller who asked for it; the weights straight into the store's buffer
    if (g.out_cov_prob)
        OEM_HIP(hipMemcpyAsync(g.out_cov_prob, d_cov, sizeof(double) * nnz, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(k_cc_weights, dim3((uint32_t)((n_reads + kCC - 1) / kCC)), dim3(kCC), 0, st, out->row_ptr, d_p, d_cov,
                       (uint32_t)n_reads, out->w64);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipStreamSynchronize(st));
    tm.lap("cov+em: weights");
    return OEM_OK;
}

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
    OEM_TRY(check_cells_coverage_args(who, bin_width, model, n_txps, nnz, n_reads));
    OEM_TRY(check_cell_row_off(who, cell_row_off, n_cells, n_reads));
    StageTimer tm;
    OEM_TRY(validate_csr(row_ptr, tid, n_reads, nnz, n_txps));
    tm.lap("cov cells: range checks");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device < 0 || device >= n_dev)
        return fail(OEM_ERR_NO_DEVICE, "%s: no HIP device %d", who, device);
    OEM_HIP(hipSetDevice(device));
    if (nnz == 0) return OEM_OK;

    // ---- chunks of consecutive cells that fit half the free HBM
    uint64_t all_bins = 0, max_nb = 0;
    for (uint32_t t = 0; t < n_txps; ++t) {
        const uint64_t nb = cov_n_bins(txp_len[t], bin_width);
        all_bins += nb;
        max_nb = std::max(max_nb, nb);
    }
    size_t free_b = 0, total_b = 0;
    OEM_HIP(hipMemGetInfo(&free_b, &total_b));
    // (per alignment: id, start, end, segment id, f64 result; per read: a u32 row pointer)
    const std::vector<Chunk> chunks = plan_chunks(cell_row_off, n_cells, row_ptr, n_txps, all_bins, max_nb, free_b / 2, 24, 4);
    uint64_t max_cells = 0, max_reads = 0, max_aln = 0;
    for (const Chunk &ch : chunks) {
        max_cells = std::max<uint64_t>(max_cells, ch.c1 - ch.c0);
        max_reads = std::max(max_reads, ch.r1 - ch.r0);
        max_aln = std::max(max_aln, ch.a1 - ch.a0);
    }
    tm.lap("cov cells: plan");

    StreamGuard sg;
    OEM_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    hipStream_t st = sg.s;
    Arena ar;
    uint32_t *d_nb, *d_tid, *d_start, *d_end, *d_rp, *d_gerr;
    uint64_t *d_len;
    double *d_out;
    OEM_TRY(ar.get(&d_len, n_txps));
    OEM_TRY(ar.get(&d_nb, n_txps));
    OEM_TRY(ar.get(&d_gerr, 1));
    OEM_TRY(ar.get(&d_tid, max_aln));
    OEM_TRY(ar.get(&d_start, max_aln));
    OEM_TRY(ar.get(&d_end, max_aln));
    OEM_TRY(ar.get(&d_out, max_aln));
    OEM_TRY(ar.get(&d_rp, max_reads + 1));
    ChunkBufs b;
    OEM_TRY(alloc_chunk_bufs(st, ar, chunks, n_txps, &b));
    uint32_t h_gerr = 0;
    OEM_TRY(setup_txps(st, txp_len, n_txps, bin_width, d_len, d_nb, d_gerr, &h_gerr));

    std::vector<uint32_t> h_rp(max_reads + 1), h_coff(max_cells + 1), h_err(max_cells);
    for (const Chunk &ch : chunks) {
        const uint32_t ncc = ch.c1 - ch.c0;
        const uint32_t nr = (uint32_t)(ch.r1 - ch.r0), na = (uint32_t)(ch.a1 - ch.a0);
        for (uint32_t c = 0; c <= ncc; ++c) h_coff[c] = (uint32_t)(row_ptr[cell_row_off[ch.c0 + c]] - ch.a0);
        for (uint64_t r = 0; r <= nr; ++r) h_rp[r] = (uint32_t)(row_ptr[ch.r0 + r] - ch.a0);
        OEM_HIP(hipMemcpyAsync(d_rp, h_rp.data(), sizeof(uint32_t) * ((size_t)nr + 1), hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(d_tid, tid + ch.a0, sizeof(uint32_t) * (size_t)na, hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(d_start, aln_start + ch.a0, sizeof(uint32_t) * (size_t)na, hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(d_end, aln_end + ch.a0, sizeof(uint32_t) * (size_t)na, hipMemcpyHostToDevice, st));
        OEM_TRY(run_chunk(st, ar, b, d_len, d_nb, n_txps, bin_width, model, growth_rate, ncc, nr, na, h_coff.data(), d_rp, 0,
                          d_tid, d_start, d_end, d_out, h_err.data()));
        if (na) {
            OEM_HIP(hipMemcpyAsync(out_cov_prob + ch.a0, d_out, sizeof(double) * (size_t)na, hipMemcpyDeviceToHost, st));
            OEM_HIP(hipStreamSynchronize(st));
        }
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
