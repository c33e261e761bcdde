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
// The three kernels run on resident arrays (coverage_body), behind two entry points: oem_coverage_probs_device
// uploads, runs them and reads the column back; oem_store_create_coverage uploads once, has k_cov_reads write the
// store's weights as well, and hands the resident CSR to the store.
// The host version manages 8 M alignments/s on one core; this one is bound by the upload of the
// alignment coordinates.
#include <cstring>
#include <new>
#include <vector>

#include "oem_coverage_common.h"
#include "oem_driver.h"

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


// The weights a store keeps for one read's alignments [b, e), from their coverage column: w = (double)p * cov, the
// expression of oem_store_create (em.rs:107-111); a read with any NaN coverage gets p * 0 on every alignment, as
// zero_nan_rows leaves it; an f32 store (weight_coding 2) gets the product rounded once to f32 (v_cvt_f32_f64 in the
// kernels' FP mode, which keeps f32 denormals: the host's (float) cast, subnormals and the underflow to 0 included).
__device__ inline void cov_read_weights(uint64_t b, uint64_t e, const float *__restrict__ p, const double *cov,
                                        double *__restrict__ w64, float *__restrict__ w32)
{
    bool nan = false;
    for (uint64_t j = b; j < e; ++j) nan |= cov[j] != cov[j];
    for (uint64_t j = b; j < e; ++j) {
        const double w = (double)p[j] * (nan ? 0.0 : cov[j]);
        if (w64) w64[j] = w;
        else w32[j] = (float)w;
    }
}

// p != NULL: the read's weights too, from the column it has just written (the store's creation path)
__global__ __launch_bounds__(kCT) void k_cov_reads(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ tid,
                                                   const uint32_t *__restrict__ aln_start, const uint32_t *__restrict__ aln_end,
                                                   const uint64_t *__restrict__ txp_len, const uint32_t *__restrict__ n_bins,
                                                   const unsigned long long *__restrict__ off,
                                                   const double *__restrict__ prob, uint64_t n_reads, double bin_length,
                                                   double *__restrict__ out, uint32_t *err, const float *__restrict__ p,
                                                   double *__restrict__ w64, float *__restrict__ w32)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t b = row_ptr[r], e = row_ptr[r + 1];
    cov_normalize_read(b, e, aln_start, aln_end, bin_length,
                       [&](uint64_t j) {
                           const uint32_t t = tid[j];
                           return CovTxpBins{prob + off[t], n_bins[t], (double)txp_len[t]};
                       },
                       out, err);
    if (p) cov_read_weights(b, e, p, out, w64, w32);
}

// The same weights in a pass of their own (the A/B against k_cov_reads' epilogue)
__global__ __launch_bounds__(kCT) void k_cov_weights(const uint32_t *__restrict__ row_ptr, const float *__restrict__ p,
                                                     const double *__restrict__ cov, uint64_t n_reads,
                                                     double *__restrict__ w64, float *__restrict__ w32)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    cov_read_weights(row_ptr[r], row_ptr[r + 1], p, cov, w64, w32);
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

// The weights a store keeps, written by the coverage pass (device arrays, nnz; p == NULL: the column only).
struct CovWeights {
    const float *p = nullptr;
    double *w64 = nullptr; // one of the two
    float *w32 = nullptr;
};

// The model on arrays already on the device (u32 row pointers, ids, coordinates, transcript lengths): the column
// into d_out, and with wt.p the store's weights.  The weights are the epilogue of k_cov_reads, or with
// OEM_COV_WEIGHTS_PASS=1 (test-only library) a pass of their own.  Bins and offsets live and die here.
int coverage_body(const uint32_t *d_rp, const uint32_t *d_tid, const uint32_t *d_start, const uint32_t *d_end,
                  const uint64_t *d_len, uint64_t n_reads, uint64_t nnz, uint32_t n_txps, uint32_t bin_width, int model,
                  double growth_rate, double *d_out, const CovWeights &wt, StageTimer *tm)
{
    Bufs bufs;
    uint32_t *d_nbins, *d_tw, *d_err;
    unsigned long long *d_off;
    OEM_TRY(bufs.get(&d_nbins, n_txps));
    OEM_TRY(bufs.get(&d_off, (size_t)n_txps + 1));
    OEM_TRY(bufs.get(&d_tw, n_txps));
    OEM_TRY(bufs.get(&d_err, 1));
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
    const bool separate = wt.p && knob("OEM_COV_WEIGHTS_PASS", 0) != 0;
    const CovWeights epi = separate ? CovWeights{} : wt;
    const dim3 rg((uint32_t)((n_reads + kCT - 1) / kCT));
    hipLaunchKernelGGL(k_cov_reads, rg, dim3(kCT), 0, 0, d_rp, d_tid, d_start, d_end, d_len, d_nbins, d_off, d_prob, n_reads,
                       (double)bin_width, d_out, d_err, epi.p, epi.w64, epi.w32);
    OEM_HIP(hipGetLastError());
    uint32_t h_err = 0;
    OEM_HIP(hipMemcpy(&h_err, d_err, sizeof(h_err), hipMemcpyDeviceToHost));
    if (tm) tm->lap(wt.p && !separate ? "cov store: coverage + weights" : "cov store: coverage");
    if (separate) {
        hipLaunchKernelGGL(k_cov_weights, rg, dim3(kCT), 0, 0, d_rp, wt.p, d_out, n_reads, wt.w64, wt.w32);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipStreamSynchronize(0));
        if (tm) tm->lap("cov store: weights");
    }
    if (h_err & kCovErrInterval) return fail(OEM_ERR_STATE, "add_interval: an alignment lies outside its transcript");
    if (h_err & kCovErrOlfrac) return fail(OEM_ERR_STATE, "coverage computation error: overlap fraction above 1");
    if (h_err & kCovErrNoBins) return fail(OEM_ERR_STATE, "a transcript has no coverage bins");
    if (h_err & kCovErrDegenerate) return fail(OEM_ERR_STATE, "degenerate coverage bin (assert, oarfish_types.rs:490)");
    if (h_err & kCovErrNonFinite) return fail(OEM_ERR_STATE, "coverage model: non-finite probability");
    return OEM_OK;
}

// The argument checks of oem_coverage_probs_device followed by those of oem_store_create, all before any device work
// (`who` names the entry point in the messages).
int check_coverage_store_args(const char *who, const uint64_t *row_ptr, const uint32_t *tid, const float *as_prob,
                              const uint32_t *aln_start, const uint32_t *aln_end, const uint64_t *txp_len,
                              uint64_t n_reads, uint64_t nnz, uint32_t n_txps, uint32_t bin_width, int model,
                              const oem_store_opts *opts)
{
    if (!row_ptr || !txp_len || (nnz && (!tid || !as_prob || !aln_start || !aln_end)))
        return fail(OEM_ERR_ARG, "%s: NULL argument", who);
    if (bin_width == 0)
        return fail(OEM_ERR_ARG, "coverage model with 0 bin width is not implemented (logistic_probability.rs:59, binomial_probability.rs:192)");
    if (model != 0 && model != 1) return fail(OEM_ERR_ARG, "%s: model must be 0 (logistic) or 1 (binomial)", who);
    if (n_txps == 0) return fail(OEM_ERR_ARG, "%s: n_txps is 0", who);
    if (nnz >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: needs nnz < 2^32", who);
    if (opts && opts->weight_coding > 2) return fail(OEM_ERR_ARG, "%s: weight_coding %u (0, 1 or 2)", who, opts->weight_coding);
    if (opts && opts->layout_build > 1) return fail(OEM_ERR_ARG, "%s: layout_build %u (0 or 1)", who, opts->layout_build);
    if (opts && opts->reorder_rows > 2) return fail(OEM_ERR_ARG, "%s: reorder_rows %u (0, 1 or 2)", who, opts->reorder_rows);
    if (row_ptr[0] != 0 || row_ptr[n_reads] != nnz) return fail(OEM_ERR_ARG, "%s: row_ptr must span [0, nnz]", who);
    return validate_csr(row_ptr, tid, n_reads, nnz, n_txps); // (non-decreasing row_ptr, tid[j] < n_txps)
}

} // namespace

int coverage_resident(const uint32_t *d_row_ptr, const uint32_t *d_tid, const uint32_t *d_start, const uint32_t *d_end,
                      const uint64_t *d_txp_len, uint64_t n_reads, uint64_t nnz, uint32_t n_txps, uint32_t bin_width,
                      int model, double growth_rate, double *d_out, const float *d_p, double *d_w64, float *d_w32)
{
    StageTimer tm;
    return coverage_body(d_row_ptr, d_tid, d_start, d_end, d_txp_len, n_reads, nnz, n_txps, bin_width, model, growth_rate,
                         d_out, CovWeights{d_p, d_w64, d_w32}, &tm);
}

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
    uint32_t *d_rp, *d_tid, *d_start, *d_end;
    uint64_t *d_len;
    double *d_out;
    OEM_TRY(bufs.get(&d_rp, n_reads + 1));
    OEM_TRY(bufs.get(&d_tid, nnz));
    OEM_TRY(bufs.get(&d_start, nnz));
    OEM_TRY(bufs.get(&d_end, nnz));
    OEM_TRY(bufs.get(&d_len, n_txps));
    OEM_TRY(bufs.get(&d_out, nnz));
    OEM_HIP(hipMemcpy(d_rp, rp32.data(), sizeof(uint32_t) * (n_reads + 1), hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_tid, tid, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_start, aln_start, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_end, aln_end, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
    OEM_HIP(hipMemcpy(d_len, txp_len, sizeof(uint64_t) * n_txps, hipMemcpyHostToDevice));
    OEM_TRY(coverage_body(d_rp, d_tid, d_start, d_end, d_len, n_reads, nnz, n_txps, bin_width, model, growth_rate, d_out,
                          CovWeights{}, nullptr));
    OEM_HIP(hipMemcpy(out_cov_prob, d_out, sizeof(double) * nnz, hipMemcpyDeviceToHost));
    return OEM_OK;
    OEM_API_END("oem_coverage_probs_device")
}

// oem_coverage_probs_device + oem_store_create on its column, with the column never on the host: the caller-order
// CSR the store adopts (row pointers narrowed on the device, ids, weights) is filled here, the coverage scratch
// (probabilities, coordinates, lengths, bins, column) is released before the layout is built.
extern "C" int oem_store_create_coverage(const uint64_t *row_ptr, const uint32_t *tid, const float *as_prob,
                                         const uint32_t *aln_start, const uint32_t *aln_end, const uint64_t *txp_len,
                                         uint64_t n_reads, uint64_t nnz, uint32_t n_txps, uint32_t bin_width, int model,
                                         double growth_rate, int device, const oem_store_opts *opts,
                                         double *out_cov_prob, oem_store **out)
{
    OEM_API_BEGIN
    const char *who = "oem_store_create_coverage";
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    StageTimer tm;
    OEM_TRY(check_coverage_store_args(who, row_ptr, tid, as_prob, aln_start, aln_end, txp_len, n_reads, nnz, n_txps,
                                      bin_width, model, opts));
    tm.lap("cov store: range checks");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device < 0 || device >= n_dev)
        return fail(OEM_ERR_NO_DEVICE, "%s: no HIP device %d", who, device);
    OEM_HIP(hipSetDevice(device));
    // weight_coding 2 (create_store_impl): the f32 store of the products rounded once, without a dictionary (coding 1)
    oem_store_opts o;
    std::memset(&o, 0, sizeof(o));
    if (opts) o = *opts;
    const bool f32w = o.weight_coding == 2;
    if (f32w) o.weight_coding = 1;

    ResidentCsr res;
    OEM_TRY(dev_alloc(&res.row_ptr, n_reads + 1, nullptr));
    OEM_TRY(dev_alloc(&res.tid, nnz, nullptr));
    if (f32w) OEM_TRY(dev_alloc(&res.w32, nnz, nullptr));
    else OEM_TRY(dev_alloc(&res.w64, nnz, nullptr));
    OEM_TRY(upload_row_ptr_u32(0, row_ptr, n_reads + 1, res.row_ptr));
    if (nnz) {
        Bufs bufs; // the coverage scratch: released at the end of this scope
        uint32_t *d_start, *d_end;
        uint64_t *d_len;
        float *d_p;
        double *d_cov;
        OEM_TRY(bufs.get(&d_p, nnz));
        OEM_TRY(bufs.get(&d_start, nnz));
        OEM_TRY(bufs.get(&d_end, nnz));
        OEM_TRY(bufs.get(&d_len, n_txps));
        OEM_TRY(bufs.get(&d_cov, nnz));
        OEM_HIP(hipMemcpy(res.tid, tid, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
        OEM_HIP(hipMemcpy(d_p, as_prob, sizeof(float) * nnz, hipMemcpyHostToDevice));
        OEM_HIP(hipMemcpy(d_start, aln_start, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
        OEM_HIP(hipMemcpy(d_end, aln_end, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
        OEM_HIP(hipMemcpy(d_len, txp_len, sizeof(uint64_t) * n_txps, hipMemcpyHostToDevice));
        tm.lap("cov store: upload");
        OEM_TRY(coverage_body(res.row_ptr, res.tid, d_start, d_end, d_len, n_reads, nnz, n_txps, bin_width, model,
                              growth_rate, d_cov, CovWeights{d_p, res.w64, res.w32}, &tm));
        if (out_cov_prob) {
            OEM_HIP(hipMemcpy(out_cov_prob, d_cov, sizeof(double) * nnz, hipMemcpyDeviceToHost));
            tm.lap("cov store: column read-back");
        }
    }
    oem_store *s = new (std::nothrow) oem_store();
    if (!s) return fail(OEM_ERR_OOM, "%s: host allocation failed", who);
    const int rc = create_store_impl(row_ptr, tid, as_prob, nullptr, n_reads, nnz, n_txps, device, &o, s, nullptr, &res);
    if (rc != OEM_OK) {
        free_store(s);
        return rc;
    }
    *out = s;
    return OEM_OK;
    OEM_API_END("oem_store_create_coverage")
}
