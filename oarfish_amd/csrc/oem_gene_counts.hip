// oem_gene_counts.hip -- the cells x transcripts CSR collapsed to cells x genes on the device (oem_cells_gene_counts).
//
// The rule is oem_gene_counts.h's: per cell and gene the entries in CSR order, added in f64 one after the other, rounded
// once to f32; an entry wherever the cell has an entry of the gene; ascending gene id inside a cell.
//
// Consecutive cells go in batches of at most kGeneBatchEntries entries (a larger cell is a batch of its own).  Per batch:
//   (upload)         the batch's slice of cell_off, its values and its cols -- the two arrays in chunks through the
//                    pinned lanes of oem_filter_device.h
//   k_gene_keys      behind every chunk of cols: per entry its cell in the batch, by binary search in the slice, and the
//                    64-bit key  cell_in_batch * n_genes + gene_of[col]  (the one random gather: 4 B of a table in L2)
//   (hipcub sort)    stable radix sort of the keys over exactly the bits in use, the f32 value as payload: inside a run
//                    of one key the values keep CSR order, so there is no index payload and no second gather
//   k_gene_heads     per entry: 1 where the key differs from the previous one (a cell boundary changes it by construction)
//   (hipcub scan)    exclusive sum of the heads: the number of the run an entry starts
//   k_gene_sums      the lane of a run's head walks the run's values in order in f64 and writes the gene id and the
//                    rounded sum at the run's number
//   k_gene_cells     the cells' offsets in the output: the scan sampled at the cells' first entries
//   (read-back)      offsets, gene ids and sums through two pinned staging buffers
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <memory>

#include "oem_cells.h"
#include "oem_filter_device.h"
#include "oem_gene_counts.h"

namespace oem {
namespace {

constexpr int kGeneBlock = 256;
constexpr uint64_t kGeneUploadChunk = 1ull << 22; // entries of an upload chunk (16 MiB)
constexpr uint64_t kGeneStageBytes = 8ull << 20;  // one of the two read-back staging buffers

// this thread's last oem_cells_gene_counts (gene_counts_last_call)
thread_local double g_gene_last[6] = {0, 0, 0, 0, 0, 0};

int gene_grid(uint64_t n)
{
    const uint64_t g = (n + kGeneBlock - 1) / kGeneBlock;
    return (int)std::min<uint64_t>(std::max<uint64_t>(g, 1), 256 * 16);
}

// One lane per entry i in [i0, i1) of the batch (entry e0 + i of the matrix).  `slice` holds the n_slice = cells + 1
// values of cell_off from the batch's first cell to the end of its last: slice[0] = e0.  The entry's cell is the last
// one whose offset is not above it (the empty cells before it share that offset and come earlier).
__global__ __launch_bounds__(kGeneBlock) void k_gene_keys(const uint64_t *__restrict__ slice, uint32_t n_slice, uint64_t e0,
                                                          const uint32_t *__restrict__ col, const uint32_t *__restrict__ gene_of,
                                                          uint32_t n_genes, uint32_t i0, uint32_t i1, uint64_t *__restrict__ key)
{
    for (uint32_t i = i0 + blockIdx.x * blockDim.x + threadIdx.x; i < i1; i += gridDim.x * blockDim.x) {
        const uint64_t e = e0 + i;
        uint32_t lo = 0, hi = n_slice; // first index whose offset is above e
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (slice[mid] <= e) lo = mid + 1;
            else hi = mid;
        }
        key[i] = (uint64_t)(lo - 1u) * n_genes + gene_of[col[i]];
    }
}

__global__ __launch_bounds__(kGeneBlock) void k_gene_heads(const uint64_t *__restrict__ key, uint32_t n, uint32_t *__restrict__ head)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}

// run[i] is the exclusive sum of head: the number of the run entry i starts when head[i] is set.  Runs are short (a
// gene's isoforms expressed in one cell), so the head's lane walks its run alone.
__global__ __launch_bounds__(kGeneBlock) void k_gene_sums(const uint64_t *__restrict__ key, const float *__restrict__ val,
                                                          const uint32_t *__restrict__ head, const uint32_t *__restrict__ run,
                                                          uint32_t n, uint32_t n_genes, uint32_t *__restrict__ out_gene,
                                                          float *__restrict__ out_val)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (!head[i]) continue;
        double acc = 0.0;
        uint32_t j = i;
        do {
            acc += (double)val[j];
            ++j;
        } while (j < n && !head[j]);
        const uint32_t r = run[i];
        out_gene[r] = (uint32_t)(key[i] % n_genes);
        out_val[r] = __double2float_rn(acc);
    }
}

// cell c of the batch starts at entry slice[c] - e0 of the batch (n for the end of the last cell: run has n + 1 entries)
__global__ __launch_bounds__(kGeneBlock) void k_gene_cells(const uint64_t *__restrict__ slice, uint32_t n_slice, uint64_t e0,
                                                           const uint32_t *__restrict__ run, uint32_t *__restrict__ cell_out)
{
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n_slice; c += gridDim.x * blockDim.x)
        cell_out[c] = run[slice[c] - e0];
}

// Device memory to the host through two pinned staging buffers: chunk k + 1 is copied down while chunk k is copied out.
struct ReadBack {
    hipStream_t st = nullptr;
    uint64_t cap = 0;
    Pinned stage[2];
    Event done[2];
    int init(hipStream_t stream, uint64_t bytes)
    {
        st = stream;
        cap = bytes;
        for (int l = 0; l < 2; ++l) {
            OEM_HIP(hipHostMalloc(&stage[l].p, cap, hipHostMallocDefault));
            OEM_HIP(hipEventCreateWithFlags(&done[l].e, hipEventDisableTiming));
        }
        return OEM_OK;
    }
    int get(void *dst, const void *d_src, uint64_t bytes)
    {
        const uint64_t n_chunks = (bytes + cap - 1) / cap;
        auto len = [&](uint64_t k) { return std::min(cap, bytes - k * cap); };
        for (uint64_t k = 0; k <= n_chunks; ++k) {
            if (k < n_chunks) {
                OEM_HIP(hipMemcpyAsync(stage[k & 1].p, (const uint8_t *)d_src + k * cap, len(k), hipMemcpyDeviceToHost, st));
                OEM_HIP(hipEventRecord(done[k & 1].e, st));
            }
            if (k >= 1) {
                OEM_HIP(hipEventSynchronize(done[(k - 1) & 1].e));
                std::memcpy((uint8_t *)dst + (k - 1) * cap, stage[(k - 1) & 1].p, len(k - 1));
            }
        }
        return OEM_OK;
    }
};

template <typename T>
int upload_chunks(const T *src, T *d_dst, const std::vector<uint64_t> &cuts)
{
    return filter_upload_measure<T>(src, d_dst, cuts.data(), cuts.size() - 1, 1, nullptr, [](hipStream_t, uint64_t, uint64_t) {});
}

std::vector<uint64_t> chunk_cuts(uint64_t n)
{
    std::vector<uint64_t> cuts;
    for (uint64_t at = 0; at < n; at += kGeneUploadChunk) cuts.push_back(at);
    cuts.push_back(n);
    return cuts;
}

int gene_counts_device(const uint64_t *cell_off, uint32_t n_cells, const uint32_t *col, const float *val, const uint32_t *gene_of,
                       uint32_t n_txps, uint32_t n_genes, std::vector<SparseBlock> *blocks)
{
    const long bk = knob("OEM_GENE_BATCH_ENTRIES", (long)kGeneBatchEntries);
    const uint64_t B = bk > 0 ? (uint64_t)bk : kGeneBatchEntries;
    std::vector<std::pair<uint32_t, uint32_t>> batches; // cells [first, second)
    uint64_t max_n = 0, max_cells = 0;
    for (uint32_t c0 = 0; c0 < n_cells;) {
        uint32_t c1 = c0 + 1;
        while (c1 < n_cells && cell_off[c1 + 1] - cell_off[c0] <= B) ++c1;
        batches.emplace_back(c0, c1);
        max_n = std::max(max_n, cell_off[c1] - cell_off[c0]);
        max_cells = std::max<uint64_t>(max_cells, c1 - c0);
        c0 = c1;
    }
    double last[6] = {0, 0, 0, 0, 0, (double)batches.size()};
    const bool timing = knob("OEM_GENE_TIMING", 0) != 0;
    auto host_ms = [](std::chrono::steady_clock::time_point t0) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    std::memcpy(g_gene_last, last, sizeof last);
    blocks->clear();
    blocks->resize(batches.size());
    for (size_t b = 0; b < batches.size(); ++b) (*blocks)[b].counts.assign(batches[b].second - batches[b].first, 0);
    if (max_n == 0) return OEM_OK;

    Stream st;
    OEM_HIP(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    DevBuf<uint32_t> d_gene_of, d_col, d_run, d_cell_out; // d_col: the cols, then (they are dead behind the keys) the heads
    DevBuf<uint64_t> d_slice, d_key[2];
    DevBuf<float> d_val[2];
    DevBuf<uint8_t> d_tmp;
    size_t tmp_cap = 0;
    uint64_t dev_bytes = 0;
    OEM_TRY(dev_alloc(&d_gene_of.p, n_txps, &dev_bytes));
    OEM_TRY(dev_alloc(&d_col.p, max_n + 1, &dev_bytes));
    OEM_TRY(dev_alloc(&d_run.p, max_n + 1, &dev_bytes));
    OEM_TRY(dev_alloc(&d_cell_out.p, max_cells + 1, &dev_bytes));
    OEM_TRY(dev_alloc(&d_slice.p, max_cells + 1, &dev_bytes));
    for (int k = 0; k < 2; ++k) {
        OEM_TRY(dev_alloc(&d_key[k].p, max_n, &dev_bytes));
        OEM_TRY(dev_alloc(&d_val[k].p, max_n, &dev_bytes));
    }
    Event ev[3]; // before the sort, behind it, behind the kernels
    if (timing)
        for (auto &e : ev) OEM_HIP(hipEventCreate(&e.e));
    OEM_TRY(upload_chunks(gene_of, d_gene_of.p, chunk_cuts(n_txps)));
    ReadBack rb;
    OEM_TRY(rb.init(st.s, std::min<uint64_t>(kGeneStageBytes, std::max<uint64_t>(4 * max_n, 4096))));

    std::vector<uint32_t> cell_out;
    for (size_t b = 0; b < batches.size(); ++b) {
        const uint32_t c0 = batches[b].first, nc = batches[b].second - c0;
        const uint64_t e0 = cell_off[c0];
        const uint32_t n = (uint32_t)(cell_off[c0 + nc] - e0); // <= 2^30: checked
        if (n == 0) continue;
        SparseBlock &blk = (*blocks)[b];
        const std::vector<uint64_t> cuts = chunk_cuts(n);
        const auto t_up = std::chrono::steady_clock::now();
        OEM_TRY(upload_chunks(cell_off + c0, d_slice.p, chunk_cuts((uint64_t)nc + 1)));
        OEM_TRY(upload_chunks(val + e0, d_val[0].p, cuts));
        OEM_TRY(filter_upload_measure<uint32_t>(col + e0, d_col.p, cuts.data(), cuts.size() - 1, 1, nullptr,
                                                [&](hipStream_t lane, uint64_t g0, uint64_t g1) {
                                                    const uint32_t i0 = (uint32_t)cuts[g0], i1 = (uint32_t)cuts[g1];
                                                    hipLaunchKernelGGL(k_gene_keys, dim3(gene_grid(i1 - i0)), dim3(kGeneBlock), 0, lane, d_slice.p,
                                                                       nc + 1u, e0, d_col.p, d_gene_of.p, n_genes, i0, i1, d_key[0].p);
                                                }));
        last[0] += host_ms(t_up);
        // the key bits in use: keys are below cells * n_genes
        const uint64_t max_key = (uint64_t)nc * n_genes - 1;
        int end_bit = 1;
        while (end_bit < 64 && (max_key >> end_bit)) ++end_bit;
        hipcub::DoubleBuffer<uint64_t> keys(d_key[0].p, d_key[1].p);
        hipcub::DoubleBuffer<float> vals(d_val[0].p, d_val[1].p);
        size_t sort_bytes = 0, scan_bytes = 0;
        OEM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys, vals, (int)n, 0, end_bit, st.s));
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)(n + 1), st.s));
        if (std::max(sort_bytes, scan_bytes) > tmp_cap) {
            d_tmp.reset();
            dev_bytes -= tmp_cap;
            tmp_cap = 0;
            OEM_TRY(dev_alloc(&d_tmp.p, std::max(sort_bytes, scan_bytes), &dev_bytes));
            tmp_cap = std::max(sort_bytes, scan_bytes);
        }
        if (timing) OEM_HIP(hipEventRecord(ev[0].e, st.s));
        OEM_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, sort_bytes, keys, vals, (int)n, 0, end_bit, st.s));
        if (timing) OEM_HIP(hipEventRecord(ev[1].e, st.s));
        uint32_t *const d_head = d_col.p;
        OEM_HIP(hipMemsetAsync(d_head + n, 0, sizeof(uint32_t), st.s));
        hipLaunchKernelGGL(k_gene_heads, dim3(gene_grid(n)), dim3(kGeneBlock), 0, st.s, keys.Current(), n, d_head);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, scan_bytes, (const uint32_t *)d_head, d_run.p, (int)(n + 1), st.s));
        // the sorted-from halves of the two double buffers are free: the batch's output
        uint32_t *const d_out_gene = reinterpret_cast<uint32_t *>(keys.Alternate());
        float *const d_out_val = vals.Alternate();
        hipLaunchKernelGGL(k_gene_sums, dim3(gene_grid(n)), dim3(kGeneBlock), 0, st.s, keys.Current(), vals.Current(), d_head, d_run.p, n,
                           n_genes, d_out_gene, d_out_val);
        OEM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_gene_cells, dim3(gene_grid((uint64_t)nc + 1)), dim3(kGeneBlock), 0, st.s, d_slice.p, nc + 1u, e0, d_run.p, d_cell_out.p);
        OEM_HIP(hipGetLastError());
        if (timing) {
            OEM_HIP(hipEventRecord(ev[2].e, st.s));
            OEM_HIP(hipEventSynchronize(ev[2].e));
            float ms = 0.f;
            OEM_HIP(hipEventElapsedTime(&ms, ev[0].e, ev[1].e));
            last[1] += ms;
            OEM_HIP(hipEventElapsedTime(&ms, ev[1].e, ev[2].e));
            last[2] += ms;
        }
        const auto t_down = std::chrono::steady_clock::now();
        cell_out.resize((size_t)nc + 1);
        OEM_TRY(rb.get(cell_out.data(), d_cell_out.p, sizeof(uint32_t) * ((size_t)nc + 1)));
        const uint32_t n_runs = cell_out[nc];
        if (n_runs == 0 || n_runs > n) return fail(OEM_ERR_STATE, "oem_cells_gene_counts: a batch of %u entries gave %u runs", n, n_runs);
        for (uint32_t c = 0; c < nc; ++c) blk.counts[c] = cell_out[c + 1] - cell_out[c];
        blk.col.resize(n_runs);
        blk.val.resize(n_runs);
        OEM_TRY(rb.get(blk.col.data(), d_out_gene, sizeof(uint32_t) * n_runs));
        OEM_TRY(rb.get(blk.val.data(), d_out_val, sizeof(float) * n_runs));
        last[3] += host_ms(t_down);
    }
    OEM_HIP(hipStreamSynchronize(st.s));
    last[4] = (double)dev_bytes;
    std::memcpy(g_gene_last, last, sizeof last);
    return OEM_OK;
}

} // namespace

void gene_counts_last_call(double *out6) { std::memcpy(out6, g_gene_last, sizeof g_gene_last); }

int gene_counts_check(const char *who, const uint64_t *cell_off, uint32_t n_cells, const uint32_t *col, const float *val,
                      const uint32_t *gene_of, uint32_t n_txps, uint32_t n_genes)
{
    if (n_cells && !cell_off) return fail(OEM_ERR_ARG, "%s: cell_off is NULL and n_cells is not 0", who);
    uint64_t nnz = 0;
    if (n_cells) {
        if (cell_off[0] != 0) return fail(OEM_ERR_ARG, "%s: cell_off[0] must be 0", who);
        for (uint32_t c = 0; c < n_cells; ++c)
            if (cell_off[c + 1] < cell_off[c]) return fail(OEM_ERR_ARG, "%s: cell_off must be non-decreasing (cell %u)", who, c);
        for (uint32_t c = 0; c < n_cells; ++c)
            if (cell_off[c + 1] - cell_off[c] > kGeneMaxCellEntries)
                return fail(OEM_ERR_ARG, "%s: cell %u has %llu entries, more than 2^30", who, c, (unsigned long long)(cell_off[c + 1] - cell_off[c]));
        nnz = cell_off[n_cells];
    }
    if (nnz && (!col || !val)) return fail(OEM_ERR_ARG, "%s: col or val is NULL and the matrix has entries", who);
    if (nnz && !gene_of) return fail(OEM_ERR_ARG, "%s: gene_of is NULL and the matrix has entries", who);
    for (uint64_t i = 0; i < nnz; ++i)
        if (col[i] >= n_txps) return fail(OEM_ERR_ARG, "%s: col[%llu] = %u is not below n_txps = %u", who, (unsigned long long)i, col[i], n_txps);
    if (gene_of)
        for (uint32_t t = 0; t < n_txps; ++t)
            if (gene_of[t] >= n_genes) return fail(OEM_ERR_ARG, "%s: gene_of[%u] = %u is not below n_genes = %u", who, t, gene_of[t], n_genes);
    return OEM_OK;
}

int gene_counts_result(const char *who, uint32_t n_cells, std::vector<SparseBlock> &blocks, oem_cells_result **out)
{
    std::unique_ptr<oem_cells_result> r(new oem_cells_result());
    r->n_cells = n_cells;
    r->infos.resize(n_cells); // zero-filled: nothing ran an EM here
    OEM_TRY(cells_result_from_blocks(who, blocks, r.get()));
    *out = r.release();
    return OEM_OK;
}

} // namespace oem

using namespace oem;

extern "C" int oem_cells_gene_counts(const uint64_t *cell_off, uint32_t n_cells, const uint32_t *col, const float *val,
                                     const uint32_t *gene_of, uint32_t n_txps, uint32_t n_genes, int device, oem_cells_result **out)
{
    OEM_API_BEGIN
    const char *who = "oem_cells_gene_counts";
    if (out) *out = nullptr;
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    OEM_TRY(gene_counts_check(who, cell_off, n_cells, col, val, gene_of, n_txps, n_genes));
    OEM_TRY(ensure_device(device));
    std::vector<SparseBlock> blocks;
    OEM_TRY(gene_counts_device(cell_off, n_cells, col, val, gene_of, n_txps, n_genes, &blocks));
    return gene_counts_result(who, n_cells, blocks, out);
    OEM_API_END("oem_cells_gene_counts")
}
