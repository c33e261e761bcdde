// oem_cells_sparse.hip -- the per-cell results as CSR on the device (oem_em_run_cells_sparse).
//
// single_cell.rs:151-160 keeps, per cell, the transcripts with count > 0.0 as (col u32, val f32) in ascending
// column order.  One 256-thread workgroup per cell walks the cell's transcripts in ascending id twice: once to count
// the entries (the host scans the counts into the cells' offsets and sizes the output), once to write them at the
// cell's offset.  Inside a chunk the order comes from a 64-bit ballot per wave, the lane's rank among the set bits
// below it, and a prefix over the four waves in LDS; a running base carries from one chunk to the next.
//
// Two source shapes: a compacted batch (rank != nullptr: transcript t of cell c sits in slot rank[c * T + t] of the
// cell's txps_eff values, kNoRank = does not occur, 0) and a dense [cell][T] vector (an uncompacted batch, or the
// count vector of one cell on the cell-by-cell path).  Ranks rise with t, so the gather of the first shape is monotone.
#include "oem_internal.h"

namespace oem {

namespace {

constexpr int kNzThreads = 256;
constexpr int kNzWaves = kNzThreads / 64;
constexpr int kNzSub = 4; // sub-chunks of 256 transcripts per step: four independent loads in flight per thread

__device__ __forceinline__ double nz_value(const CellsNzSource &src, uint32_t c, uint32_t t)
{
    if (src.rank) {
        const uint32_t r = src.rank[(size_t)c * src.T + t];
        return r == kNoRank ? 0.0 : src.v[(size_t)c * src.stride + r];
    }
    return src.v[(size_t)c * src.stride + t];
}

// number of lanes below this one whose bit is set in `mask`
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ __launch_bounds__(kNzThreads) void k_cells_nz_count(CellsNzSource src, uint32_t n_cells, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t part[kNzWaves];
    const uint32_t c = blockIdx.x;
    if (c >= n_cells) return;
    uint32_t n = 0;
    for (uint32_t t = threadIdx.x; t < src.T; t += kNzThreads)
        n += nz_value(src, c, t) > 0.0 ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int w = 0; w < kNzWaves; ++w) total += part[w];
        counts[c] = total;
    }
}

// off[c] .. off[c + 1]: cell c's entries (the host's scan of k_cells_nz_count); a write past off[c + 1] is dropped
// (it cannot happen: both kernels read the same values with the same test)
__global__ __launch_bounds__(kNzThreads) void k_cells_nz_emit(CellsNzSource src, uint32_t n_cells, const uint64_t *__restrict__ off,
                                                              uint32_t *__restrict__ col, float *__restrict__ val)
{
    __shared__ uint32_t part[2][kNzSub][kNzWaves]; // two buffers: one barrier per step
    const uint32_t c = blockIdx.x;
    if (c >= n_cells) return;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t end = off[c + 1];
    uint64_t base = off[c];
    uint32_t buf = 0;
    for (uint32_t t0 = 0; t0 < src.T; t0 += kNzSub * kNzThreads, buf ^= 1u) {
        double v[kNzSub];
#pragma unroll
        for (int k = 0; k < kNzSub; ++k) {
            const uint32_t t = t0 + k * kNzThreads + threadIdx.x;
            v[k] = t < src.T ? nz_value(src, c, t) : 0.0;
        }
        uint32_t below[kNzSub];
#pragma unroll
        for (int k = 0; k < kNzSub; ++k) {
            const uint64_t mask = __ballot(v[k] > 0.0);
            below[k] = lanes_below(mask);
            if (lane == 0) part[buf][k][wave] = (uint32_t)__popcll(mask);
        }
        __syncthreads();
        uint32_t before = 0; // entries of this step ahead of the current (sub-chunk, wave)
#pragma unroll
        for (int k = 0; k < kNzSub; ++k) {
            uint32_t mine = before;
            for (int w = 0; w < kNzWaves; ++w) {
                const uint32_t n = part[buf][k][w];
                mine += w < (int)wave ? n : 0u;
                before += n;
            }
            const uint64_t i = base + mine + below[k];
            if (v[k] > 0.0 && i < end) {
                col[i] = t0 + k * kNzThreads + threadIdx.x;
                val[i] = __double2float_rn(v[k]); // round to nearest even, denormals kept (Rust's `as f32`)
            }
        }
        base += before;
    }
}

} // namespace

int launch_cells_nz_count(hipStream_t st, const CellsNzSource &src, uint32_t n_cells, uint32_t *d_counts)
{
    if (n_cells == 0) return OEM_OK;
    hipLaunchKernelGGL(k_cells_nz_count, dim3(n_cells), dim3(kNzThreads), 0, st, src, n_cells, d_counts);
    OEM_HIP(hipGetLastError());
    return OEM_OK;
}

int launch_cells_nz_emit(hipStream_t st, const CellsNzSource &src, uint32_t n_cells, const uint64_t *d_off, uint32_t *d_col,
                         float *d_val)
{
    if (n_cells == 0) return OEM_OK;
    hipLaunchKernelGGL(k_cells_nz_emit, dim3(n_cells), dim3(kNzThreads), 0, st, src, n_cells, d_off, d_col, d_val);
    OEM_HIP(hipGetLastError());
    return OEM_OK;
}

} // namespace oem
