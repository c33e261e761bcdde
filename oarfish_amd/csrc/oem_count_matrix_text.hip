// oem_count_matrix_text.hip -- the `.count.mtx` file of the single-cell path, formatted on the device
// (oem_count_matrix_text).
//
// Reference: write_function::write_single_cell_output (src/util/write_function.rs:53-54) hands the cells x transcripts
// matrix to sprs::io::write_matrix_market: a banner, a dimension line, then one line per stored entry,
//     row + 1 ' ' col + 1 ' ' value '\n'
// with the f32 value printed by `{}` (oem_shortest_f32.h).  The caller passes the banner and the dimension line as
// `prefix`; the entries come as the CSR that oem_em_cells_sparse and the session return.
//
// The entries are walked in chunks of consecutive entries, at most as many as a device text buffer holds lines of the
// greatest length.  Per chunk, on one of two lanes (a stream with its entry and text buffers):
//   (upload)        the chunk's cols and values (8 B per entry) and its slice of cell_off
//   k_mtx_measure   per entry: its cell, by binary search in the slice -> its row number and the line's length
//   (hipcub scan)   lengths -> u64 byte offsets of the lines inside the chunk
//   k_mtx_emit      per workgroup 256 consecutive entries: the lines written into an LDS stage, the stage copied to the
//                   text buffer with aligned 16-byte stores (dwords, then bytes, at its two unaligned ends)
//   (read-back)     the offsets, and -- once the host knows from them where the chunk's text goes -- the text
// The read-back of chunk c is enqueued when the kernels of chunk c + 1 are already running on the other lane.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <memory>

#include "oem_driver.h"
#include "oem_shortest_f32.h"

namespace oem {
namespace {

constexpr int kMtxBlock = 256;
// row and column are u32 (10 digits), the value is a sign and kShortestF32MaxLen - 1 bytes, two blanks and the newline
constexpr uint32_t kMtxMaxLine = 10 + 1 + 10 + 1 + kShortestF32MaxLen + 1;
// the stage of a workgroup: its lines, shifted by the text's address modulo 16 so that aligned words of the stage are
// aligned words of the text
constexpr uint32_t kMtxStageBytes = (kMtxBlock * kMtxMaxLine + 15 + 15) / 16 * 16;
static_assert(kMtxStageBytes >= kMtxBlock * (10 + 1 + 10 + 1 + kShortestF32MaxLen + 1) + 15, "the stage holds 256 lines of the greatest length at any shift");
static_assert(kMtxStageBytes <= 64 * 1024, "the stage is static LDS");
constexpr uint64_t kMtxBufBytes = 256ull << 20; // a device text buffer (the test-only library: OEM_MTX_BUF_BYTES)
constexpr uint64_t kMtxMaxChunk = 1ull << 30;   // entries of a chunk (the scan counts in int)

thread_local float g_mtx_ms[3] = {0.f, 0.f, 0.f}; // measure, scan, emit of this thread's last call (OEM_MTX_TIMING)

// One lane per entry i of the chunk (entry e0 + i of the matrix).  `slice` holds the n_slice values of cell_off from
// the cell of the chunk's first entry to the end of the cell of its last: slice[0] <= e0 and slice[n_slice - 1] > the
// last entry.  The entry's cell is the last one whose offset is not above it (the empty cells before it share that
// offset and come earlier); its row number is row0 + that index.
__global__ __launch_bounds__(kMtxBlock) void k_mtx_measure(const uint64_t *__restrict__ slice, uint32_t n_slice, uint64_t e0,
                                                           uint32_t row0, const uint32_t *__restrict__ col,
                                                           const uint32_t *__restrict__ val, uint32_t n,
                                                           uint32_t *__restrict__ row, uint32_t *__restrict__ len)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t e = e0 + i;
        uint32_t lo = 0, hi = n_slice; // first index whose offset is above e
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (slice[mid] <= e) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t r = row0 + (lo - 1u);
        row[i] = r;
        len[i] = u32_dec_len(r) + 1u + u32_dec_len(col[i] + 1u) + 1u + shortest_f32_len(val[i]) + 1u;
    }
}

// One workgroup per tile of kMtxBlock consecutive entries (tiles beyond the grid in further rounds).  The tile's lines
// are the bytes [off[first], off[last]) of `out`: each lane writes its line into the stage, then all lanes copy the
// stage out.  Stage byte s stands for the byte (out + off[first]) - shift + s, shift = that address modulo 16.
__global__ __launch_bounds__(kMtxBlock) void k_mtx_emit(const uint32_t *__restrict__ row, const uint32_t *__restrict__ col,
                                                        const uint32_t *__restrict__ val, const uint64_t *__restrict__ off,
                                                        uint32_t n, uint8_t *__restrict__ out)
{
    __shared__ uint4 stage4[kMtxStageBytes / 16];
    uint8_t *const stage = reinterpret_cast<uint8_t *>(stage4);
    const uint32_t n_tiles = (n + kMtxBlock - 1) / kMtxBlock;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t first = t * kMtxBlock;
        const uint32_t last = min(first + (uint32_t)kMtxBlock, n);
        const uint64_t base = off[first];
        const uint32_t bytes = (uint32_t)(off[last] - base); // <= kMtxBlock * kMtxMaxLine
        uint8_t *const dst = out + base;
        const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
        const uint32_t i = first + threadIdx.x;
        if (i < last) {
            uint8_t *p = stage + shift + (uint32_t)(off[i] - base);
            p = emit_u32(p, row[i]);
            *p++ = ' ';
            p = emit_u32(p, col[i] + 1u);
            *p++ = ' ';
            p = emit_shortest_f32(p, val[i]);
            *p = '\n';
        }
        __syncthreads();
        // the stage's bytes [s0, s1): bytes up to a dword boundary, dwords up to a 16-byte boundary, 16-byte words, and
        // the same in reverse at the end (every range may be empty; a short tile may have no aligned word at all)
        uint8_t *const dst0 = dst - shift; // 16-byte aligned; nothing below dst is written
        const uint32_t s0 = shift, s1 = shift + bytes;
        const uint32_t a4 = min((s0 + 3u) & ~3u, s1);
        const uint32_t b4 = max(s1 & ~3u, a4);
        const uint32_t a16 = min((a4 + 15u) & ~15u, b4);
        const uint32_t b16 = max(b4 & ~15u, a16);
        for (uint32_t s = a16 + 16u * threadIdx.x; s < b16; s += 16u * kMtxBlock)
            *reinterpret_cast<uint4 *>(dst0 + s) = stage4[s / 16u];
        {
            const uint32_t *const stage1 = reinterpret_cast<const uint32_t *>(stage4);
            uint32_t s = a4 + 4u * threadIdx.x;
            if (s < a16) *reinterpret_cast<uint32_t *>(dst0 + s) = stage1[s / 4u];
            s = b16 + 4u * threadIdx.x;
            if (s < b4) *reinterpret_cast<uint32_t *>(dst0 + s) = stage1[s / 4u];
            s = s0 + threadIdx.x;
            if (s < a4) dst0[s] = stage[s];
            s = b4 + threadIdx.x;
            if (s < s1) dst0[s] = stage[s];
        }
        __syncthreads(); // the stage is written again in the next round
    }
}

// at most 256 * 16 workgroups (the test-only library: OEM_MTX_GRID_BLOCKS, so that a small matrix takes several rounds)
int mtx_grid(uint64_t n)
{
    const long cap = knob("OEM_MTX_GRID_BLOCKS", 256 * 16);
    const uint64_t g = (n + kMtxBlock - 1) / kMtxBlock;
    return (int)std::min<uint64_t>(std::max<uint64_t>(g, 1), (uint64_t)std::max(cap, 1L));
}

struct U32ToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

// One of the two lanes: a stream, the buffers of the chunk that runs on it, and that chunk while it is in flight.
struct MtxLane {
    hipStream_t stream = nullptr;
    uint32_t *col = nullptr, *val = nullptr, *row = nullptr, *len = nullptr;
    uint64_t *off = nullptr;
    uint8_t *text = nullptr, *tmp = nullptr;
    uint64_t *slice = nullptr;
    uint64_t slice_cap = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // before measure, after it, after the scan, after emit
    bool busy = false;
    uint64_t e0 = 0, e1 = 0;
    MtxLane() = default;
    MtxLane(const MtxLane &) = delete;
    MtxLane &operator=(const MtxLane &) = delete;
    ~MtxLane()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        (void)hipFree(col);
        (void)hipFree(val);
        (void)hipFree(row);
        (void)hipFree(len);
        (void)hipFree(off);
        (void)hipFree(text);
        (void)hipFree(tmp);
        (void)hipFree(slice);
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

int count_matrix_text(const uint64_t *cell_off, uint32_t n_cells, const uint32_t *col, const float *val, uint32_t row_base,
                      const uint8_t *prefix, uint64_t prefix_len, oem_text_result *res)
{
    const uint64_t nnz = n_cells ? cell_off[n_cells] : 0;
    res->n_lines = res->n_kept = nnz;
    res->line_off.assign(nnz + 1, 0);
    res->kept.assign(nnz, 1u);
    if (nnz == 0) {
        res->n_bytes = prefix_len;
        res->text.reset(new uint8_t[prefix_len ? prefix_len : 1]);
        if (prefix_len) std::memcpy(res->text.get(), prefix, prefix_len);
        return OEM_OK;
    }
    const bool timing = knob("OEM_MTX_TIMING", 0) != 0;
    const long cap_knob = knob("OEM_MTX_BUF_BYTES", (long)kMtxBufBytes);
    const uint64_t cap = cap_knob > 0 ? (uint64_t)cap_knob : kMtxBufBytes;
    // entries of a chunk: their lines fit the text buffer whatever they hold (one entry at the least: the smallest
    // buffer is one line of the greatest length)
    const uint64_t E = std::min(std::min(std::max<uint64_t>(cap / kMtxMaxLine, 1), kMtxMaxChunk), nnz);

    MtxLane lanes[2];
    size_t tmp_bytes = 0;
    {
        hipcub::TransformInputIterator<uint64_t, U32ToU64, const uint32_t *> in(nullptr, U32ToU64());
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, in, (uint64_t *)nullptr, (int)(E + 1), (hipStream_t) nullptr));
    }
    for (auto &ln : lanes) {
        OEM_HIP(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
        OEM_TRY(dev_alloc(&ln.col, E, nullptr));
        OEM_TRY(dev_alloc(&ln.val, E, nullptr));
        OEM_TRY(dev_alloc(&ln.row, E, nullptr));
        OEM_TRY(dev_alloc(&ln.len, E + 1, nullptr));
        OEM_TRY(dev_alloc(&ln.off, E + 1, nullptr));
        OEM_TRY(dev_alloc(&ln.text, E * kMtxMaxLine, nullptr));
        OEM_TRY(dev_alloc(&ln.tmp, tmp_bytes, nullptr));
        if (timing)
            for (auto &e : ln.ev) OEM_HIP(hipEventCreate(&e));
        if (nnz <= E) break; // one chunk: one lane
    }

    // The host text.  Its size is known only when the last chunk is measured, so it is sized from the lines measured so
    // far (their mean length for the entries still to come, and a sixteenth more) and grows if that falls short.
    uint64_t text_cap = 0;
    auto reserve_text = [&](uint64_t done, uint64_t body_bytes, uint64_t body_have) -> int {
        const uint64_t need = prefix_len + body_bytes;
        if (need <= text_cap) return OEM_OK;
        const uint64_t mean = (body_bytes + done - 1) / done;
        const uint64_t rest = (nnz - done) * mean;
        const uint64_t want = need + rest + rest / 16 + (done < nnz ? 4096 : 0);
        for (auto &ln : lanes) // the copies into the text so far
            if (ln.stream) OEM_HIP(hipStreamSynchronize(ln.stream));
        std::unique_ptr<uint8_t[]> grown(new uint8_t[want]);
        if (res->text) std::memcpy(grown.get(), res->text.get(), prefix_len + body_have);
        else if (prefix_len) std::memcpy(grown.get(), prefix, prefix_len);
        res->text = std::move(grown);
        text_cap = want;
        return OEM_OK;
    };

    float ms[3] = {0.f, 0.f, 0.f};
    // the chunk in flight on a lane: its offsets have arrived once its stream is idle; they place its text
    auto finish = [&](MtxLane &ln) -> int {
        if (!ln.busy) return OEM_OK;
        ln.busy = false;
        OEM_HIP(hipStreamSynchronize(ln.stream));
        uint64_t *lo = res->line_off.data();
        const uint64_t base = lo[ln.e0]; // (the chunk before this one is finished: final)
        for (uint64_t i = ln.e0 + 1; i <= ln.e1; ++i) lo[i] += base;
        OEM_TRY(reserve_text(ln.e1, lo[ln.e1], base));
        const uint64_t bytes = lo[ln.e1] - base;
        if (bytes) OEM_HIP(hipMemcpyAsync(res->text.get() + prefix_len + base, ln.text, bytes, hipMemcpyDeviceToHost, ln.stream));
        if (timing) {
            for (int k = 0; k < 3; ++k) {
                float t = 0.f;
                OEM_HIP(hipEventElapsedTime(&t, ln.ev[k], ln.ev[k + 1]));
                ms[k] += t;
            }
        }
        return OEM_OK;
    };

    const uint64_t *const off_end = cell_off + n_cells + 1;
    uint64_t e0 = 0;
    for (uint32_t c = 0; e0 < nnz; ++c) {
        const uint64_t e1 = std::min(e0 + E, nnz);
        const uint32_t n = (uint32_t)(e1 - e0);
        MtxLane &ln = lanes[c & 1];
        // cell_off from the cell of entry e0 to the first offset above entry e1 - 1
        const uint64_t c0 = (uint64_t)(std::upper_bound(cell_off, off_end, e0) - cell_off) - 1;
        const uint64_t c1 = (uint64_t)(std::upper_bound(cell_off + c0, off_end, e1 - 1) - cell_off);
        const uint64_t n_slice = c1 - c0 + 1;
        if (n_slice > ln.slice_cap) {
            OEM_HIP(hipStreamSynchronize(ln.stream));
            (void)hipFree(ln.slice);
            ln.slice = nullptr;
            ln.slice_cap = 0;
            OEM_TRY(dev_alloc(&ln.slice, n_slice, nullptr));
            ln.slice_cap = n_slice;
        }
        OEM_HIP(hipMemcpyAsync(ln.slice, cell_off + c0, sizeof(uint64_t) * n_slice, hipMemcpyHostToDevice, ln.stream));
        OEM_HIP(hipMemcpyAsync(ln.col, col + e0, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ln.stream));
        OEM_HIP(hipMemcpyAsync(ln.val, val + e0, sizeof(float) * n, hipMemcpyHostToDevice, ln.stream));
        OEM_HIP(hipMemsetAsync(ln.len + n, 0, sizeof(uint32_t), ln.stream));
        if (timing) OEM_HIP(hipEventRecord(ln.ev[0], ln.stream));
        hipLaunchKernelGGL(k_mtx_measure, dim3(mtx_grid(n)), dim3(kMtxBlock), 0, ln.stream, ln.slice, (uint32_t)n_slice, e0,
                           (uint32_t)(row_base + c0 + 1), ln.col, ln.val, n, ln.row, ln.len);
        OEM_HIP(hipGetLastError());
        if (timing) OEM_HIP(hipEventRecord(ln.ev[1], ln.stream));
        {
            hipcub::TransformInputIterator<uint64_t, U32ToU64, const uint32_t *> in(ln.len, U32ToU64());
            size_t tb = tmp_bytes;
            OEM_HIP(hipcub::DeviceScan::ExclusiveSum(ln.tmp, tb, in, ln.off, (int)(n + 1), ln.stream));
        }
        if (timing) OEM_HIP(hipEventRecord(ln.ev[2], ln.stream));
        hipLaunchKernelGGL(k_mtx_emit, dim3(mtx_grid(n)), dim3(kMtxBlock), 0, ln.stream, ln.row, ln.col, ln.val, ln.off, n, ln.text);
        OEM_HIP(hipGetLastError());
        if (timing) OEM_HIP(hipEventRecord(ln.ev[3], ln.stream));
        // the ends of the chunk's lines, relative to the chunk (finish() makes them offsets into the body)
        OEM_HIP(hipMemcpyAsync(res->line_off.data() + e0 + 1, ln.off + 1, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, ln.stream));
        ln.busy = true;
        ln.e0 = e0;
        ln.e1 = e1;
        // the previous chunk's text comes back while this chunk's kernels run
        OEM_TRY(finish(lanes[(c & 1) ^ 1]));
        e0 = e1;
    }
    OEM_TRY(finish(lanes[0])); // (one of the two is in flight: the last chunk)
    OEM_TRY(finish(lanes[1]));
    for (auto &ln : lanes)
        if (ln.stream) OEM_HIP(hipStreamSynchronize(ln.stream));
    res->n_bytes = prefix_len + res->line_off[nnz];
    if (timing) std::memcpy(g_mtx_ms, ms, sizeof ms);
    return OEM_OK;
}

} // namespace

void mtx_last_timing(float *ms3) { std::memcpy(ms3, g_mtx_ms, sizeof g_mtx_ms); }

} // namespace oem

using namespace oem;

extern "C" int oem_count_matrix_text(const uint64_t *cell_off, uint32_t n_cells, const uint32_t *col, const float *val,
                                     uint32_t n_txps, uint32_t row_base, const uint8_t *prefix, uint64_t prefix_len, int device,
                                     oem_text_result **out)
{
    OEM_API_BEGIN
    if (out) *out = nullptr;
    if (!out) return fail(OEM_ERR_ARG, "oem_count_matrix_text: out is NULL");
    if (n_cells && !cell_off) return fail(OEM_ERR_ARG, "oem_count_matrix_text: cell_off is NULL and n_cells is not 0");
    if (!prefix && prefix_len) return fail(OEM_ERR_ARG, "oem_count_matrix_text: prefix is NULL and prefix_len is not 0");
    if ((uint64_t)row_base + n_cells > 0xffffffffull)
        return fail(OEM_ERR_ARG, "oem_count_matrix_text: row_base + n_cells = %llu is above 2^32 - 1", (unsigned long long)row_base + n_cells);
    uint64_t nnz = 0;
    if (n_cells) {
        if (cell_off[0] != 0) return fail(OEM_ERR_ARG, "oem_count_matrix_text: cell_off[0] must be 0");
        for (uint32_t c = 0; c < n_cells; ++c)
            if (cell_off[c + 1] < cell_off[c]) return fail(OEM_ERR_ARG, "oem_count_matrix_text: cell_off must be non-decreasing (cell %u)", c);
        nnz = cell_off[n_cells];
    }
    if (nnz && (!col || !val)) return fail(OEM_ERR_ARG, "oem_count_matrix_text: col or val is NULL and the matrix has entries");
    for (uint64_t i = 0; i < nnz; ++i)
        if (col[i] >= n_txps)
            return fail(OEM_ERR_ARG, "oem_count_matrix_text: col[%llu] = %u is not below n_txps = %u", (unsigned long long)i, col[i], n_txps);
    OEM_TRY(ensure_device(device));
    std::unique_ptr<oem_text_result> res(new oem_text_result);
    OEM_TRY(count_matrix_text(cell_off, n_cells, col, val, row_base, prefix, prefix_len, res.get()));
    res->content_bytes = res->n_bytes;
    *out = res.release();
    return OEM_OK;
    OEM_API_END("oem_count_matrix_text")
}
