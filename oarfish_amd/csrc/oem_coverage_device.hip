// oem_coverage_device.hip -- the coverage model on the device.
//
// Same arithmetic, in f64, as the host restatement in oem_builder.cpp (which follows
// TranscriptInfo::add_interval, src/util/oarfish_types.rs:496-538; logistic_prob,
// src/util/logistic_probability.rs:7-79; binomial_continuous_prob, src/util/binomial_probability.rs:7-224;
// normalize_read_probs, src/util/normalize_probability.rs:5-74):
//
//   k_cov_bins       one thread per alignment: overlap fraction of every coverage bin it spans,
//                    added with f64 atomics (the host adds in store order: sums agree to ~1e-16)
//   k_cov_bin_probs  one thread per transcript: min coverage, f32 counts, logistic or binomial
//                    bin probabilities (sequential over the transcript's bins, as on the host)
//   k_cov_reads      one thread per read: per-alignment coverage probability, normalised per read
//
// The arithmetic itself lives in oem_coverage_common.h, shared with the per-cell kernels of oem_coverage_cells.hip.
// The host version manages 8 M alignments/s on one core; this one is bound by the upload of the
// alignment coordinates.
#include "oem_coverage_common.h"
#include "oem_internal.h"

namespace oem {

namespace {

constexpr int kCT = 256;

__global__ __launch_bounds__(kCT) void k_cov_bin_counts(const uint64_t *__restrict__ txp_len, uint32_t n_txps,
                                                        uint32_t bin_width, uint32_t *__restrict__ n_bins)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_txps) return;
    n_bins[t] = cov_n_bins(txp_len[t], bin_width); // with_len_and_bin_width (:460-468)
}

// exclusive prefix sum of n_bins (one workgroup; T <= 2^32 but this is O(T / 1024) per thread)
__global__ __launch_bounds__(1024) void k_cov_bin_offsets(const uint32_t *__restrict__ n_bins, uint32_t n_txps,
                                                          unsigned long long *__restrict__ off /* [T + 1] */)
{
    __shared__ unsigned long long part[1024];
    const uint32_t per = (n_txps + blockDim.x - 1) / blockDim.x;
    const uint32_t b = threadIdx.x * per, e = min(n_txps, b + per);
    unsigned long long s = 0;
    for (uint32_t i = b; i < e; ++i) s += n_bins[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long acc = 0;
        for (uint32_t i = 0; i < blockDim.x; ++i) { const unsigned long long v = part[i]; part[i] = acc; acc += v; }
        off[n_txps] = acc;
    }
    __syncthreads();
    s = part[threadIdx.x];
    for (uint32_t i = b; i < e; ++i) { off[i] = s; s += n_bins[i]; }
}

__global__ __launch_bounds__(kCT) void k_cov_bins(const uint32_t *__restrict__ tid, const uint32_t *__restrict__ aln_start,
                                                  const uint32_t *__restrict__ aln_end, const uint64_t *__restrict__ txp_len,
                                                  const uint32_t *__restrict__ n_bins,
                                                  const unsigned long long *__restrict__ off, uint64_t nnz,
                                                  double *__restrict__ bins, uint32_t *__restrict__ total_weight,
                                                  uint32_t *err)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nnz) return;
    const uint32_t t = tid[j];
    if (!cov_add_interval(aln_start[j], aln_end[j], n_bins[t], (double)txp_len[t], bins + off[t], err)) return;
    atomicAdd(&total_weight[t], 1u);                                               // :537 (weight 1.0, :727)
}

__global__ __launch_bounds__(kCT) void k_cov_bin_probs(const uint64_t *__restrict__ txp_len, const uint32_t *__restrict__ n_bins,
                                                       const unsigned long long *__restrict__ off,
                                                       const uint32_t *__restrict__ total_weight, uint32_t n_txps,
                                                       int model, double growth_rate, double *__restrict__ bins,
                                                       double *__restrict__ prob, uint32_t *err)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_txps) return;
    cov_bin_probs(bins + off[t], prob + off[t], n_bins[t], (double)txp_len[t], total_weight[t], model, growth_rate, err);
}

__global__ __launch_bounds__(kCT) void k_cov_reads(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ tid,
                                                   const uint32_t *__restrict__ aln_start, const uint32_t *__restrict__ aln_end,
                                                   const uint64_t *__restrict__ txp_len, const uint32_t *__restrict__ n_bins,
                                                   const unsigned long long *__restrict__ off,
                                                   const double *__restrict__ prob, uint64_t n_reads, double bin_length,
                                                   double *__restrict__ out, uint32_t *err)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    cov_normalize_read(row_ptr[r], row_ptr[r + 1], aln_start, aln_end, bin_length,
                       [&](uint64_t j) {
                           const uint32_t t = tid[j];
                           return CovTxpBins{prob + off[t], n_bins[t], (double)txp_len[t]};
                       },
                       out, err);
}

struct Bufs {
    std::vector<void *> p;
    template <typename T> int get(T **q, size_t n)
    {
        *q = nullptr;
        hipError_t e = hipMalloc((void **)q, (n ? n : 1) * sizeof(T));
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? OEM_ERR_OOM : OEM_ERR_HIP, "coverage model: %s", hipGetErrorString(e));
        p.push_back(*q);
        return OEM_OK;
    }
    ~Bufs() { for (void *q : p) hipFree(q); }
};

} // namespace
} // namespace oem

using namespace oem;

extern "C" int oem_coverage_probs_device(const uint64_t *row_ptr, const uint32_t *tid, const uint32_t *aln_start,
                                         const uint32_t *aln_end, const uint64_t *txp_len, uint64_t n_reads,
                                         uint64_t nnz, uint32_t n_txps, uint32_t bin_width, int model,
                                         double growth_rate, int device, double *out_cov_prob)
{
    OEM_API_BEGIN
    if (!row_ptr || !txp_len || (nnz && (!tid || !aln_start || !aln_end || !out_cov_prob)))
        return fail(OEM_ERR_ARG, "oem_coverage_probs_device: NULL argument");
    if (bin_width == 0)
        return fail(OEM_ERR_ARG, "coverage model with 0 bin width is not implemented (logistic_probability.rs:59, binomial_probability.rs:192)");
    if (model != 0 && model != 1) return fail(OEM_ERR_ARG, "oem_coverage_probs_device: model must be 0 (logistic) or 1 (binomial)");
    if (n_txps == 0) return fail(OEM_ERR_ARG, "oem_coverage_probs_device: n_txps is 0");
    if (nnz >= (1ull << 32)) return fail(OEM_ERR_ARG, "oem_coverage_probs_device: needs nnz < 2^32");
    if (row_ptr[0] != 0 || row_ptr[n_reads] != nnz) return fail(OEM_ERR_ARG, "oem_coverage_probs_device: row_ptr must span [0, nnz]");
    for (uint64_t j = 0; j < nnz; ++j)
        if (tid[j] >= n_txps) return fail(OEM_ERR_ARG, "tid[%llu]=%u is not below n_txps=%u", (unsigned long long)j, tid[j], n_txps);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device < 0 || device >= n_dev)
        return fail(OEM_ERR_NO_DEVICE, "oem_coverage_probs_device: no HIP device %d", device);
    OEM_HIP(hipSetDevice(device));
    if (nnz == 0) return OEM_OK;

    Bufs bufs;
    std::vector<uint32_t> rp32(n_reads + 1);
    for (uint64_t i = 0; i <= n_reads; ++i) rp32[i] = (uint32_t)row_ptr[i];
    uint32_t *d_rp, *d_tid, *d_start, *d_end, *d_nbins, *d_tw, *d_err;
    uint64_t *d_len;
    unsigned long long *d_off;
    double *d_out;
    OEM_TRY(bufs.get(&d_rp, n_reads + 1));
    OEM_TRY(bufs.get(&d_tid, nnz));
    OEM_TRY(bufs.get(&d_start, nnz));
    OEM_TRY(bufs.get(&d_end, nnz));
    OEM_TRY(bufs.get(&d_len, n_txps));
    OEM_TRY(bufs.get(&d_nbins, n_txps));
    OEM_TRY(bufs.get(&d_off, (size_t)n_txps + 1));
    OEM_TRY(bufs.get(&d_tw, n_txps));
    OEM_TRY(bufs.get(&d_err, 1));
    OEM_TRY(bufs.get(&d_out, nnz));
    OEM_HIP(hipMemcpy(d_rp, rp32.data(), sizeof(uint32_t) * (n_reads + 1), hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_tid, tid, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_start, aln_start, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_end, aln_end, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_len, txp_len, sizeof(uint64_t) * n_txps, hipMemcpyHostToDevice));
    OEM_HIP(hipMemset(d_tw, 0, sizeof(uint32_t) * n_txps));
    OEM_HIP(hipMemset(d_err, 0, sizeof(uint32_t)));

    const uint32_t tg = (n_txps + kCT - 1) / kCT;
    hipLaunchKernelGGL(k_cov_bin_counts, dim3(tg), dim3(kCT), 0, 0, d_len, n_txps, bin_width, d_nbins);
    hipLaunchKernelGGL(k_cov_bin_offsets, dim3(1), dim3(1024), 0, 0, d_nbins, n_txps, d_off);
    unsigned long long total_bins = 0;
    OEM_HIP(hipMemcpy(&total_bins, d_off + n_txps, sizeof(total_bins), hipMemcpyDeviceToHost));
    double *d_bins, *d_prob;
    OEM_TRY(bufs.get(&d_bins, total_bins));
    OEM_TRY(bufs.get(&d_prob, total_bins));
    OEM_HIP(hipMemset(d_bins, 0, sizeof(double) * (total_bins ? total_bins : 1)));
    hipLaunchKernelGGL(k_cov_bins, dim3((uint32_t)((nnz + kCT - 1) / kCT)), dim3(kCT), 0, 0, d_tid, d_start, d_end, d_len,
                       d_nbins, d_off, nnz, d_bins, d_tw, d_err);
    hipLaunchKernelGGL(k_cov_bin_probs, dim3(tg), dim3(kCT), 0, 0, d_len, d_nbins, d_off, d_tw, n_txps, model, growth_rate,
                       d_bins, d_prob, d_err);
    hipLaunchKernelGGL(k_cov_reads, dim3((uint32_t)((n_reads + kCT - 1) / kCT)), dim3(kCT), 0, 0, d_rp, d_tid, d_start, d_end,
                       d_len, d_nbins, d_off, d_prob, n_reads, (double)bin_width, d_out, d_err);
    OEM_HIP(hipGetLastError());
    uint32_t h_err = 0;
    OEM_HIP(hipMemcpy(&h_err, d_err, sizeof(h_err), hipMemcpyDeviceToHost));
    if (h_err & kCovErrInterval) return fail(OEM_ERR_STATE, "add_interval: an alignment lies outside its transcript");
    if (h_err & kCovErrOlfrac) return fail(OEM_ERR_STATE, "coverage computation error: overlap fraction above 1");
    if (h_err & kCovErrNoBins) return fail(OEM_ERR_STATE, "a transcript has no coverage bins");
    if (h_err & kCovErrDegenerate) return fail(OEM_ERR_STATE, "degenerate coverage bin (assert, oarfish_types.rs:490)");
    if (h_err & kCovErrNonFinite) return fail(OEM_ERR_STATE, "coverage model: non-finite probability");
    OEM_HIP(hipMemcpy(out_cov_prob, d_out, sizeof(double) * nnz, hipMemcpyDeviceToHost));
    return OEM_OK;
    OEM_API_END("oem_coverage_probs_device")
}
