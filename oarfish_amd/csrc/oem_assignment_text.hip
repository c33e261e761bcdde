// oem_assignment_text.hip -- the body of the `.prob` file, formatted on the device (oem_assignment_text).
//
// Reference: write_function::write_out_prob (src/util/write_function.rs:283-332), one line per read:
//     name '\t' k '\t' id_1 '\t' .. id_k '\t' p_1 '\t' .. p_k '\n'        (k = 0: name "\t0\t\t\n")
// The arithmetic is k_assignment_probs' (oem_kernels.hip), the text comes from oem_text_format.h.  Three steps:
//   k_text_measure   per read: the E-step once -> denom, denom2, k and the line's length in bytes
//   (hipcub scan)    lengths -> u64 byte offsets of the lines (they are the result's line_off)
//   k_text_emit      per read: the line written at its offset; nprob is recomputed from denom, p from denom2, by the
//                    function the measure kernel ran (line_nprob), so the two agree bit for bit
// The text leaves the device in chunks of consecutive reads that fit a device text buffer; two buffers on two streams,
// so that the read-back of chunk c runs while chunk c + 1 is being written.
//
// oem_assignment_text_lz4 is the same call with one more step per chunk: the chunk's text (after the caller's prefix, in
// the first chunk) is compressed where it lies (oem_lz4.hip: blocks, scan, gather), and only the chunk's part of the
// LZ4 frame is read back.  The host learns that part's length from the device; it waits for it when the next chunk's
// kernels are already enqueued on the other stream.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "oem_driver.h"
#include "oem_lz4.h"
#include "oem_text_format.h"

namespace oem {
namespace {

constexpr int kTextBlock = 256;
constexpr uint64_t kTextBufBytes = 256ull << 20; // a device text buffer (the test-only library: OEM_TEXT_BUF_BYTES)

thread_local float g_text_ms[3] = {0.f, 0.f, 0.f}; // measure, scan, emit of this thread's last call (OEM_TEXT_TIMING)
thread_local float g_text_lz4_ms[2] = {0.f, 0.f};  // k_lz4_blocks, scan + k_lz4_gather of its last compressed call

// write_function.rs:307 as k_assignment_probs computes it: clamp keeps NaN, and NaN is never kept (:309)
template <typename WT>
__device__ __forceinline__ double line_nprob(const double *__restrict__ counts, const uint32_t *__restrict__ tid,
                                             const WT *__restrict__ w, uint64_t j, double denom)
{
    double nprob = (counts[tid[j]] * (double)w[j]) / denom;
    if (nprob < 0.0) nprob = 0.0;
    if (nprob > 1.0) nprob = 1.0;
    return nprob;
}

// One lane per read.  len[r] = bytes of the read's line, kept[r] = its k.
template <typename PtrT, typename WT>
__global__ __launch_bounds__(kTextBlock) void k_text_measure(const PtrT *__restrict__ row_ptr, const uint32_t *__restrict__ tid,
                                                             const WT *__restrict__ w, const double *__restrict__ counts,
                                                             uint64_t n_reads, double display_thresh, uint32_t decimals,
                                                             const uint32_t *__restrict__ name_len, double *__restrict__ denom_out,
                                                             double *__restrict__ denom2_out, uint32_t *__restrict__ kept,
                                                             uint32_t *__restrict__ len)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = row_ptr[r], e = row_ptr[r + 1];
        double denom = 0.0;
        for (uint64_t j = b; j < e; ++j) denom += counts[tid[j]] * (double)w[j]; // :286-291
        double denom2 = 0.0;
        uint32_t k = 0, bytes = 0;
        for (uint64_t j = b; j < e; ++j) { // :303-314
            const double nprob = line_nprob(counts, tid, w, j, denom);
            if (nprob >= display_thresh) {
                ++k;
                bytes += u32_dec_len(tid[j]);
                denom2 += nprob;
            }
        }
        // (not k * (decimals + 2): a kept -0.0 prints its sign, 0 / 0 prints NaN)
        for (uint64_t j = b; j < e; ++j) { // :316-318
            const double nprob = line_nprob(counts, tid, w, j, denom);
            if (nprob >= display_thresh) bytes += fixed_len(nprob / denom2, decimals);
        }
        // name \t k \t ids \t probs \n, each list joined by k - 1 tabs
        bytes += (name_len ? name_len[r] : 0u) + 4u + u32_dec_len(k) + (k ? 2u * (k - 1u) : 0u);
        denom_out[r] = denom;
        denom2_out[r] = denom2;
        kept[r] = k;
        len[r] = bytes;
    }
}

// One lane per read of the chunk [r0, r1): the line at out + (off[r] - off[r0]).  `names` holds the chunk's names from
// byte name_off[0] of the caller's blob on; name_off is the chunk's slice of the caller's offsets.
template <typename PtrT, typename WT>
__global__ __launch_bounds__(kTextBlock) void k_text_emit(const PtrT *__restrict__ row_ptr, const uint32_t *__restrict__ tid,
                                                          const WT *__restrict__ w, const double *__restrict__ counts, uint64_t r0,
                                                          uint64_t r1, double display_thresh, uint32_t decimals,
                                                          const uint8_t *__restrict__ names, const uint64_t *__restrict__ name_off,
                                                          const uint32_t *__restrict__ name_len, const double *__restrict__ denom_in,
                                                          const double *__restrict__ denom2_in, const uint32_t *__restrict__ kept,
                                                          const uint64_t *__restrict__ off, uint8_t *__restrict__ out)
{
    const uint64_t base = off[r0];
    for (uint64_t r = r0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < r1; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = row_ptr[r], e = row_ptr[r + 1];
        const double denom = denom_in[r], denom2 = denom2_in[r];
        uint8_t *p = out + (off[r] - base);
        if (name_len) {
            const uint8_t *src = names + (name_off[r - r0] - name_off[0]);
            const uint32_t n = name_len[r];
            for (uint32_t i = 0; i < n; ++i) p[i] = src[i];
            p += n;
        }
        *p++ = '\t';
        p = emit_u32(p, kept[r]);
        *p++ = '\t';
        bool first = true;
        for (uint64_t j = b; j < e; ++j) {
            if (line_nprob(counts, tid, w, j, denom) >= display_thresh) {
                if (!first) *p++ = '\t';
                first = false;
                p = emit_u32(p, tid[j]);
            }
        }
        *p++ = '\t';
        first = true;
        for (uint64_t j = b; j < e; ++j) {
            const double nprob = line_nprob(counts, tid, w, j, denom);
            if (nprob >= display_thresh) {
                if (!first) *p++ = '\t';
                first = false;
                p = emit_fixed(p, nprob / denom2, decimals);
            }
        }
        *p = '\n';
    }
}

// grid-stride kernels: at most 256 * 16 workgroups (the test-only library: OEM_TEXT_GRID_BLOCKS, so that a small store
// takes more than one stride)
int text_grid(uint64_t n)
{
    const long cap = knob("OEM_TEXT_GRID_BLOCKS", 256 * 16);
    const uint64_t g = (n + kTextBlock - 1) / kTextBlock;
    return (int)std::min<uint64_t>(std::max<uint64_t>(g, 1), (uint64_t)std::max(cap, 1L));
}

struct U32ToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

// write_function.rs:218-224
uint32_t prob_display_decimals(double display_thresh)
{
    if (display_thresh > 0.0 && std::isfinite(display_thresh))
        return (uint32_t)std::min(std::max(std::ceil(-std::log10(display_thresh)), 3.0), 9.0);
    return 9;
}

// What one of the two text buffers owns: the stream its chunks run on, the text and the chunk's names.
struct TextLane {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint8_t *text = nullptr;
    uint64_t text_cap = 0;
    uint8_t *names = nullptr;
    uint64_t names_cap = 0;
    uint64_t *name_off = nullptr;
    uint64_t name_off_cap = 0;
    // the chunk in flight: its text goes to host_dst once its kernel is done
    uint8_t *host_dst = nullptr;
    uint64_t bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the compressed call: the chunk's blocks, and whether their read-back is still to be enqueued
    Lz4Chunk lz;
    bool lz_pending = false;
    hipEvent_t ev2 = nullptr, ev3 = nullptr; // after k_lz4_blocks, after k_lz4_gather
    TextLane() = default;
    TextLane(const TextLane &) = delete;
    TextLane &operator=(const TextLane &) = delete;
    ~TextLane()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        (void)hipFree(text);
        (void)hipFree(names);
        (void)hipFree(name_off);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev2) (void)hipEventDestroy(ev2);
        if (ev3) (void)hipEventDestroy(ev3);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

// a device buffer of at least `need` elements; the lane's stream is idle when it is replaced
template <typename T>
int lane_reserve(TextLane &ln, T **buf, uint64_t *cap, uint64_t need)
{
    if (need <= *cap && *buf) return OEM_OK;
    OEM_HIP(hipStreamSynchronize(ln.stream));
    (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    OEM_TRY(dev_alloc(buf, (size_t)need, nullptr));
    *cap = need;
    return OEM_OK;
}

int lane_read_back(TextLane &ln)
{
    if (ln.bytes) OEM_HIP(hipMemcpyAsync(ln.host_dst, ln.text, ln.bytes, hipMemcpyDeviceToHost, ln.stream));
    ln.bytes = 0;
    return OEM_OK;
}

// The compressed call's part of the frame that a lane's chunk made: waits for the chunk (the other lane's kernels are
// enqueued by now), then enqueues the read-back of exactly its bytes behind the frame so far.
int lane_read_back_lz4(TextLane &ln, oem_text_result *res, uint64_t *frame_at)
{
    if (!ln.lz_pending) return OEM_OK;
    ln.lz_pending = false;
    OEM_HIP(hipStreamSynchronize(ln.stream));
    const uint64_t bytes = ln.lz.h_info[0];
    if (bytes) OEM_HIP(hipMemcpyAsync(res->text.get() + *frame_at, ln.lz.frame, bytes, hipMemcpyDeviceToHost, ln.stream));
    *frame_at += bytes;
    res->n_blocks += ln.lz.n_blocks;
    res->raw_blocks += ln.lz.h_info[1];
    return OEM_OK;
}

// oem_assignment_text_lz4: the bytes ahead of the body
struct Lz4Prefix {
    const uint8_t *bytes = nullptr;
    uint64_t len = 0;
};

// the reads [r0, r1) of the chunk that starts at r0: those whose lines fit `budget` bytes, one read at the least
uint64_t chunk_end(const std::vector<uint64_t> &off, uint64_t r0, uint64_t budget)
{
    const uint64_t r1 = (uint64_t)(std::upper_bound(off.begin() + r0, off.end(), off[r0] + budget) - off.begin()) - 1;
    return r1 <= r0 ? r0 + 1 : r1;
}

int assignment_text(oem_store *s, const double *counts, double display_thresh, const uint8_t *names, const uint64_t *name_off,
                    const std::vector<uint32_t> &name_len, oem_text_result *res, const Lz4Prefix *lz = nullptr)
{
    const DeviceCsr &m = s->csr;
    const uint64_t R = m.n_reads;
    res->n_lines = R;
    res->line_off.assign(R + 1, 0);
    res->kept.assign(R, 0);
    if (R == 0) {
        if (lz) { // a frame of the prefix alone
            res->content_bytes = lz->len;
            OEM_TRY(lz4_frame_from_host(lz->bytes, lz->len, s->stream, &res->text, &res->n_bytes, &res->n_blocks, &res->raw_blocks));
        }
        return OEM_OK;
    }
    if (R > 0x7ffffffeull) return fail(OEM_ERR_STATE, "oem_assignment_text: %llu reads in one store (the scan takes 2^31 - 2)", (unsigned long long)R);
    const uint32_t decimals = prob_display_decimals(display_thresh);
    const bool timing = knob("OEM_TEXT_TIMING", 0) != 0;
    hipStream_t st = s->stream;

    DevBuf<double> d_denom, d_denom2;
    DevBuf<uint32_t> d_kept, d_len, d_name_len;
    DevBuf<uint64_t> d_off;
    DevBuf<uint8_t> d_tmp;
    OEM_TRY(dev_alloc(&d_denom.p, R, nullptr));
    OEM_TRY(dev_alloc(&d_denom2.p, R, nullptr));
    OEM_TRY(dev_alloc(&d_kept.p, R, nullptr));
    OEM_TRY(dev_alloc(&d_len.p, R + 1, nullptr));
    OEM_TRY(dev_alloc(&d_off.p, R + 1, nullptr));
    if (names) {
        OEM_TRY(dev_alloc(&d_name_len.p, R, nullptr));
        OEM_HIP(hipMemcpyAsync(d_name_len.p, name_len.data(), sizeof(uint32_t) * R, hipMemcpyHostToDevice, st));
    }
    OEM_HIP(hipMemcpyAsync(s->theta, counts, sizeof(double) * m.n_txps, hipMemcpyHostToDevice, st));
    OEM_HIP(hipMemsetAsync(d_len.p + R, 0, sizeof(uint32_t), st));

    TextLane lanes[2];
    lanes[0].stream = st;
    OEM_HIP(hipStreamCreateWithFlags(&lanes[1].stream, hipStreamNonBlocking));
    lanes[1].own_stream = true;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    struct EvGuard {
        hipEvent_t *e;
        ~EvGuard()
        {
            for (int i = 0; i < 3; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } ev_guard{ev};
    if (timing) {
        for (auto &e : ev) OEM_HIP(hipEventCreate(&e));
        for (auto &ln : lanes) {
            OEM_HIP(hipEventCreate(&ln.ev0));
            OEM_HIP(hipEventCreate(&ln.ev1));
            if (lz) {
                OEM_HIP(hipEventCreate(&ln.ev2));
                OEM_HIP(hipEventCreate(&ln.ev3));
            }
        }
        OEM_HIP(hipEventRecord(ev[0], st));
    }

    // -- measure ------------------------------------------------------------------------------------------------
#define OEM_TEXT_DISPATCH(LAUNCH)                                      \
    do {                                                               \
        if (m.wide_ptr) {                                              \
            if (m.w_is_f64) LAUNCH(uint64_t, double, (const double *)m.w64); \
            else LAUNCH(uint64_t, float, (const float *)m.w32);        \
        } else {                                                       \
            if (m.w_is_f64) LAUNCH(uint32_t, double, (const double *)m.w64); \
            else LAUNCH(uint32_t, float, (const float *)m.w32);        \
        }                                                              \
    } while (0)
#define OEM_LAUNCH_MEASURE(PT, WT, wptr)                                                                               \
    hipLaunchKernelGGL((k_text_measure<PT, WT>), dim3(text_grid(R)), dim3(kTextBlock), 0, st, (const PT *)m.row_ptr, m.tid, \
                       wptr, s->theta, R, display_thresh, decimals, d_name_len.p, d_denom.p, d_denom2.p, d_kept.p, d_len.p)
    OEM_TEXT_DISPATCH(OEM_LAUNCH_MEASURE);
#undef OEM_LAUNCH_MEASURE
    OEM_HIP(hipGetLastError());
    if (timing) OEM_HIP(hipEventRecord(ev[1], st));

    // -- scan: u32 lengths summed in u64 ----------------------------------------------------------------------------
    {
        hipcub::TransformInputIterator<uint64_t, U32ToU64, const uint32_t *> in(d_len.p, U32ToU64());
        size_t tmp_bytes = 0;
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, in, d_off.p, (int)(R + 1), st));
        OEM_TRY(dev_alloc(&d_tmp.p, tmp_bytes, nullptr));
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, in, d_off.p, (int)(R + 1), st));
    }
    if (timing) OEM_HIP(hipEventRecord(ev[2], st));
    OEM_HIP(hipMemcpyAsync(res->line_off.data(), d_off.p, sizeof(uint64_t) * (R + 1), hipMemcpyDeviceToHost, st));
    OEM_HIP(hipMemcpyAsync(res->kept.data(), d_kept.p, sizeof(uint32_t) * R, hipMemcpyDeviceToHost, st));
    OEM_HIP(hipStreamSynchronize(st));
    const std::vector<uint64_t> &off = res->line_off;
    for (uint32_t k : res->kept) res->n_kept += k;
    const long cap_knob = knob("OEM_TEXT_BUF_BYTES", (long)kTextBufBytes);
    const uint64_t cap = cap_knob > 0 ? (uint64_t)cap_knob : kTextBufBytes;
    // the compressed call: the prefix lies in the first chunk's buffer ahead of the body, and takes its room there (a
    // prefix longer than the buffer grows it for that chunk, as a single long line does)
    const uint64_t prefix_len = lz ? lz->len : 0;
    const uint64_t first_budget = cap > prefix_len ? cap - prefix_len : 0;
    const uint32_t lz_block = lz ? lz4_block_bytes() : 0;
    const uint64_t text_bytes = prefix_len + off[R];
    uint64_t frame_at = lz4::kFrameHeaderBytes; // (the compressed call) the frame so far
    if (lz) {
        // the content size is known here, before any text exists; so is every chunk, and with them the frame's bound
        uint64_t n_blocks = 0;
        for (uint64_t a = 0, c = 0; a < R; ++c) {
            const uint64_t b = chunk_end(off, a, c ? cap : first_budget);
            n_blocks += lz4_blocks_of((c ? 0 : prefix_len) + off[b] - off[a], lz_block);
            a = b;
        }
        res->content_bytes = text_bytes;
        res->text.reset(new uint8_t[lz4::kFrameHeaderBytes + text_bytes + lz4::kBlockOverheadBytes * n_blocks + lz4::kEndMarkBytes]);
        lz4::frame_header(res->text.get(), text_bytes);
    } else {
        res->n_bytes = off[R];
        res->text.reset(new uint8_t[res->n_bytes ? res->n_bytes : 1]);
    }

    // -- emit, chunk by chunk -------------------------------------------------------------------------------------------
    float emit_ms = 0.f, lz_ms[2] = {0.f, 0.f};
    // a lane's last chunk, once its events are complete
    auto lane_times = [&](TextLane &ln) { // (a lane that never ran a chunk has no times: not an error)
        float ms[3] = {0.f, 0.f, 0.f};
        if (hipEventElapsedTime(&ms[0], ln.ev0, ln.ev1) != hipSuccess) return;
        if (lz && (hipEventElapsedTime(&ms[1], ln.ev1, ln.ev2) != hipSuccess || hipEventElapsedTime(&ms[2], ln.ev2, ln.ev3) != hipSuccess)) return;
        emit_ms += ms[0];
        lz_ms[0] += ms[1];
        lz_ms[1] += ms[2];
    };
    uint64_t r0 = 0;
    for (uint32_t c = 0; r0 < R; ++c) {
        // the reads whose lines fit the buffer; a single line longer than it grows the buffer for this chunk
        const uint64_t r1 = chunk_end(off, r0, c ? cap : first_budget);
        const uint64_t bytes = off[r1] - off[r0];
        const uint64_t pre = c ? 0 : prefix_len;
        TextLane &ln = lanes[c & 1];
        TextLane &prev = lanes[(c & 1) ^ 1];
        if (timing && c >= 2) { // the lane's previous chunk, before its events are recorded again
            OEM_HIP(hipEventSynchronize(lz ? ln.ev3 : ln.ev1));
            lane_times(ln);
        }
        OEM_TRY(lane_reserve(ln, &ln.text, &ln.text_cap, std::max(pre + bytes, std::min(cap, text_bytes))));
        if (pre) OEM_HIP(hipMemcpyAsync(ln.text, lz->bytes, pre, hipMemcpyHostToDevice, ln.stream));
        if (names) {
            const uint64_t nb = name_off[r1] - name_off[r0];
            OEM_TRY(lane_reserve(ln, &ln.names, &ln.names_cap, nb));
            OEM_TRY(lane_reserve(ln, &ln.name_off, &ln.name_off_cap, r1 - r0));
            if (nb) OEM_HIP(hipMemcpyAsync(ln.names, names + name_off[r0], nb, hipMemcpyHostToDevice, ln.stream));
            OEM_HIP(hipMemcpyAsync(ln.name_off, name_off + r0, sizeof(uint64_t) * (r1 - r0), hipMemcpyHostToDevice, ln.stream));
        }
        if (timing) OEM_HIP(hipEventRecord(ln.ev0, ln.stream));
#define OEM_LAUNCH_EMIT(PT, WT, wptr)                                                                                    \
    hipLaunchKernelGGL((k_text_emit<PT, WT>), dim3(text_grid(r1 - r0)), dim3(kTextBlock), 0, ln.stream,                  \
                       (const PT *)m.row_ptr, m.tid, wptr, s->theta, r0, r1, display_thresh, decimals, ln.names, ln.name_off, \
                       d_name_len.p, d_denom.p, d_denom2.p, d_kept.p, d_off.p, ln.text + pre)
        OEM_TEXT_DISPATCH(OEM_LAUNCH_EMIT);
#undef OEM_LAUNCH_EMIT
        OEM_HIP(hipGetLastError());
        if (timing) OEM_HIP(hipEventRecord(ln.ev1, ln.stream));
        if (lz) {
            OEM_TRY(lz4_chunk_enqueue(ln.lz, ln.text, pre + bytes, lz_block, ln.stream, ln.ev2, ln.ev3));
            ln.lz_pending = true;
            // the previous chunk's blocks come back while this chunk's kernels run
            OEM_TRY(lane_read_back_lz4(prev, res, &frame_at));
        } else {
            ln.host_dst = res->text.get() + off[r0];
            ln.bytes = bytes;
            // the previous chunk's text comes back while this chunk's kernel runs
            OEM_TRY(lane_read_back(prev));
        }
        r0 = r1;
    }
#undef OEM_TEXT_DISPATCH
    if (lz) { // (one of the two is pending: the last chunk's)
        OEM_TRY(lane_read_back_lz4(lanes[0], res, &frame_at));
        OEM_TRY(lane_read_back_lz4(lanes[1], res, &frame_at));
        std::memset(res->text.get() + frame_at, 0, lz4::kEndMarkBytes);
        res->n_bytes = frame_at + lz4::kEndMarkBytes;
    } else {
        OEM_TRY(lane_read_back(lanes[0]));
        OEM_TRY(lane_read_back(lanes[1]));
    }
    OEM_HIP(hipStreamSynchronize(lanes[0].stream));
    OEM_HIP(hipStreamSynchronize(lanes[1].stream));
    if (timing) {
        for (auto &ln : lanes) {
            if (hipEventQuery(lz ? ln.ev3 : ln.ev1) == hipSuccess) lane_times(ln);
            (void)hipGetLastError();
        }
        OEM_HIP(hipEventElapsedTime(&g_text_ms[0], ev[0], ev[1]));
        OEM_HIP(hipEventElapsedTime(&g_text_ms[1], ev[1], ev[2]));
        g_text_ms[2] = emit_ms;
        if (lz) std::memcpy(g_text_lz4_ms, lz_ms, sizeof lz_ms);
    }
    return OEM_OK;
}

} // namespace

void text_last_timing(float *ms3) { std::memcpy(ms3, g_text_ms, sizeof g_text_ms); }
void text_lz4_last_timing(float *ms2) { std::memcpy(ms2, g_text_lz4_ms, sizeof g_text_lz4_ms); }

} // namespace oem

using namespace oem;

namespace {

// what the two entry points share: the argument checks (before any device use), the lock, the result
int assignment_text_call(const char *who, oem_store *s, const double *counts, double display_thresh, const uint8_t *names,
                         const uint64_t *name_off, const Lz4Prefix *lz, oem_text_result **out)
{
    if (out) *out = nullptr;
    if (!s || !counts || !out) return fail(OEM_ERR_ARG, "%s: NULL argument", who);
    if ((names == nullptr) != (name_off == nullptr))
        return fail(OEM_ERR_ARG, "%s: names and name_off come together (both NULL: empty names)", who);
    if (lz && !lz->bytes && lz->len) return fail(OEM_ERR_ARG, "%s: prefix is NULL and prefix_len is not 0", who);
    const uint64_t R = s->csr.n_reads;
    std::vector<uint32_t> name_len;
    if (names) {
        if (name_off[0] != 0) return fail(OEM_ERR_ARG, "%s: name_off[0] must be 0", who);
        name_len.resize(R);
        for (uint64_t r = 0; r < R; ++r) {
            if (name_off[r + 1] < name_off[r]) return fail(OEM_ERR_ARG, "%s: name_off must be non-decreasing (read %llu)", who, (unsigned long long)r);
            uint64_t n = name_off[r + 1] - name_off[r];
            if (n > 0xffffffffull) return fail(OEM_ERR_ARG, "%s: name of read %llu is longer than 2^32 - 1 bytes", who, (unsigned long long)r);
            const uint8_t *p = names + name_off[r];
            while (n && p[n - 1] == 0) --n; // trim_end_matches('\0'), write_function.rs:294
            name_len[r] = (uint32_t)n;
        }
    }
    std::lock_guard<std::mutex> lk(s->mu);
    OEM_TRY(ensure_device(s->device));
    std::unique_ptr<oem_text_result> res(new oem_text_result);
    OEM_TRY(assignment_text(s, counts, display_thresh, names, name_off, name_len, res.get(), lz));
    if (!lz) res->content_bytes = res->n_bytes;
    *out = res.release();
    return OEM_OK;
}

} // namespace

extern "C" int oem_assignment_text(oem_store *s, const double *counts, double display_thresh, const uint8_t *names,
                                   const uint64_t *name_off, oem_text_result **out)
{
    OEM_API_BEGIN
    return assignment_text_call("oem_assignment_text", s, counts, display_thresh, names, name_off, nullptr, out);
    OEM_API_END("oem_assignment_text")
}

extern "C" int oem_assignment_text_lz4(oem_store *s, const double *counts, double display_thresh, const uint8_t *names,
                                       const uint64_t *name_off, const uint8_t *prefix, uint64_t prefix_len, oem_text_result **out)
{
    OEM_API_BEGIN
    Lz4Prefix lz;
    lz.bytes = prefix;
    lz.len = prefix_len;
    return assignment_text_call("oem_assignment_text_lz4", s, counts, display_thresh, names, name_off, &lz, out);
    OEM_API_END("oem_assignment_text_lz4")
}

extern "C" int oem_text_result_info(const oem_text_result *r, uint32_t key, uint64_t *value)
{
    if (!r || !value) return fail(OEM_ERR_ARG, "oem_text_result_info: NULL argument");
    switch (key) {
    case OEM_TEXT_INFO_CONTENT_BYTES: *value = r->content_bytes; return OEM_OK;
    case OEM_TEXT_INFO_BLOCKS: *value = r->n_blocks; return OEM_OK;
    case OEM_TEXT_INFO_RAW_BLOCKS: *value = r->raw_blocks; return OEM_OK;
    }
    return fail(OEM_ERR_ARG, "oem_text_result_info: unknown key %u", key);
}

extern "C" int oem_text_result_dims(const oem_text_result *r, uint64_t *n_bytes, uint64_t *n_lines, uint64_t *n_kept)
{
    if (!r) return fail(OEM_ERR_ARG, "oem_text_result_dims: NULL result");
    if (n_bytes) *n_bytes = r->n_bytes;
    if (n_lines) *n_lines = r->n_lines;
    if (n_kept) *n_kept = r->n_kept;
    return OEM_OK;
}

extern "C" int oem_text_result_copy(const oem_text_result *r, uint8_t *text, uint64_t *line_off, uint32_t *kept)
{
    if (!r) return fail(OEM_ERR_ARG, "oem_text_result_copy: NULL result");
    if (text && r->n_bytes) std::memcpy(text, r->text.get(), r->n_bytes);
    if (line_off) std::memcpy(line_off, r->line_off.data(), sizeof(uint64_t) * r->line_off.size());
    if (kept && !r->kept.empty()) std::memcpy(kept, r->kept.data(), sizeof(uint32_t) * r->kept.size());
    return OEM_OK;
}

extern "C" void oem_text_result_destroy(oem_text_result *r)
{
    delete r;
}
