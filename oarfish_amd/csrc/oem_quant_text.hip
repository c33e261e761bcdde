// oem_quant_text.hip -- the per-transcript text files of the bulk path, formatted on the device: `.quant`
// (oem_quant_text) and `.ambig_info.tsv` (oem_ambig_text).
//
// Reference: write_function::write_output (src/util/write_function.rs:104-145) writes, after a header line each,
//     name '\t' len '\t' count '\n'                 per transcript into `.quant`, the f64 count printed by `{}`
//                                                    (oem_shortest_f64.h), and
//     unique '\t' total - unique '\t' total '\n'    per transcript into `.ambig_info.tsv` (the difference saturating).
// The caller passes the header line as `prefix`.
//
// Both files go through one pair of kernels, instantiated for a description of the file's lines (QuantLines,
// AmbigLines: the length of line i, and its bytes).  The lines are walked in chunks of consecutive transcripts: as
// many as fit a device text buffer at the greatest length each could have (a chunk always holds whole lines; a line
// that would straddle the buffer's end opens the next chunk).  Per chunk, on one of two lanes (a stream with its
// input and text buffers):
//   (upload)         the chunk's columns (`.quant`: its names and their offsets, lens, counts)
//   k_lines_measure  per line: its length
//   (hipcub scan)    lengths -> u64 byte offsets of the lines inside the chunk
//   k_lines_emit     per workgroup 256 consecutive lines: written into an LDS stage, the stage copied to the text buffer
//                    with aligned 16-byte stores (dwords, then bytes, at its two unaligned ends).  Lines vary in length
//                    far more than those of `.count.mtx` -- a name has any length, a count's text up to 327 bytes -- so
//                    the stage is sized for ordinary lines (128 bytes each on average), and a workgroup whose lines do
//                    not fit it writes them straight to the text buffer instead.
//   (read-back)      the offsets, and -- once the host knows from them where the chunk's text goes -- the text
// The read-back of chunk c is enqueued when the kernels of chunk c + 1 are already running on the other lane.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "oem_driver.h"
#include "oem_shortest_f64.h"

namespace oem {
namespace {

constexpr int kQtBlock = 256;
// the stage of a workgroup: its lines, shifted by the text's address modulo 16 so that aligned words of the stage are
// aligned words of the text
constexpr uint32_t kQtStageBytes = 32 * 1024;
constexpr uint32_t kQtStageLines = kQtStageBytes - 15; // bytes of lines the stage holds at any shift
static_assert(kQtStageBytes % 16 == 0 && kQtStageBytes <= 64 * 1024, "the stage is static LDS, a whole number of 16-byte words");
constexpr uint64_t kQtBufBytes = 256ull << 20; // a device text buffer (the test-only library: OEM_QUANT_BUF_BYTES)
constexpr uint64_t kQtMaxChunk = 1ull << 30;   // lines of a chunk (the scan counts in int, the kernels in u32)

// chunks, tiles staged, tiles written directly, then ms of measure, scan, emit (OEM_QUANT_TIMING) of this thread's
// last call
thread_local double g_quant_last[6] = {0, 0, 0, 0, 0, 0};

// -- the two line descriptions: device views of a chunk's columns -------------------------------------------------------
// `.quant`: names holds the chunk's names from byte name_off[0] of the caller's blob on; name_off is the chunk's slice
// of the caller's offsets (one more than lines).
struct QuantLines {
    const uint8_t *names;
    const uint64_t *name_off;
    const uint64_t *lens;
    const uint64_t *counts; // the bits of the f64
    // what follows the name, at its longest: a tab, a u64 (20 digits), a tab, the count, the newline
    static constexpr uint64_t kMaxTail = 1 + 20 + 1 + kShortestF64MaxLen + 1;
    __device__ uint64_t len(uint32_t i) const
    {
        return (name_off[i + 1] - name_off[i]) + 1u + u64_dec_len(lens[i]) + 1u + shortest_f64_len(counts[i]) + 1u;
    }
    __device__ void emit(uint8_t *p, uint32_t i) const
    {
        const uint8_t *src = names + (name_off[i] - name_off[0]);
        const uint64_t nl = name_off[i + 1] - name_off[i];
        for (uint64_t k = 0; k < nl; ++k) p[k] = src[k];
        p += nl;
        *p++ = '\t';
        p = emit_u64(p, lens[i]);
        *p++ = '\t';
        p = emit_shortest_f64(p, counts[i]);
        *p = '\n';
    }
};

// `.ambig_info.tsv`
struct AmbigLines {
    const uint32_t *unique;
    const uint32_t *total;
    static constexpr uint64_t kMaxLine = 3 * (10 + 1);
    __device__ static uint32_t ambig(uint32_t u, uint32_t t) { return t > u ? t - u : 0u; } // saturating_sub
    __device__ uint64_t len(uint32_t i) const
    {
        const uint32_t u = unique[i], t = total[i];
        return u32_dec_len(u) + 1u + u32_dec_len(ambig(u, t)) + 1u + u32_dec_len(t) + 1u;
    }
    __device__ void emit(uint8_t *p, uint32_t i) const
    {
        const uint32_t u = unique[i], t = total[i];
        p = emit_u32(p, u);
        *p++ = '\t';
        p = emit_u32(p, ambig(u, t));
        *p++ = '\t';
        p = emit_u32(p, t);
        *p = '\n';
    }
};

// One lane per line i of the chunk.
template <class Lines>
__global__ __launch_bounds__(kQtBlock) void k_lines_measure(Lines lines, uint32_t n, uint64_t *__restrict__ len)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) len[i] = lines.len(i);
}

// One workgroup per tile of kQtBlock consecutive lines (tiles beyond the grid in further rounds).  The tile's lines are
// the bytes [off[first], off[last]) of `out`.  Where they fit the stage each lane writes its line into it, then all
// lanes copy the stage out: stage byte s stands for the byte (out + off[first]) - shift + s, shift = that address
// modulo 16.  Where they do not (one decision per workgroup: the barriers stay uniform), each lane writes its line to
// `out` itself.
template <class Lines>
__global__ __launch_bounds__(kQtBlock) void k_lines_emit(Lines lines, const uint64_t *__restrict__ off, uint32_t n,
                                                         uint8_t *__restrict__ out)
{
    __shared__ uint4 stage4[kQtStageBytes / 16];
    uint8_t *const stage = reinterpret_cast<uint8_t *>(stage4);
    const uint32_t n_tiles = (n + kQtBlock - 1) / kQtBlock;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t first = t * kQtBlock;
        const uint32_t last = min(first + (uint32_t)kQtBlock, n);
        const uint64_t base = off[first];
        const uint64_t tile_bytes = off[last] - base;
        const uint32_t i = first + threadIdx.x;
        if (tile_bytes > kQtStageLines) {
            if (i < last) lines.emit(out + off[i], i);
            continue;
        }
        const uint32_t bytes = (uint32_t)tile_bytes;
        uint8_t *const dst = out + base;
        const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
        if (i < last) lines.emit(stage + shift + (uint32_t)(off[i] - base), i);
        __syncthreads();
        // the stage's bytes [s0, s1): bytes up to a dword boundary, dwords up to a 16-byte boundary, 16-byte words, and
        // the same in reverse at the end (every range may be empty; a short tile may have no aligned word at all)
        uint8_t *const dst0 = dst - shift; // 16-byte aligned; nothing below dst is written
        const uint32_t s0 = shift, s1 = shift + bytes;
        const uint32_t a4 = min((s0 + 3u) & ~3u, s1);
        const uint32_t b4 = max(s1 & ~3u, a4);
        const uint32_t a16 = min((a4 + 15u) & ~15u, b4);
        const uint32_t b16 = max(b4 & ~15u, a16);
        for (uint32_t s = a16 + 16u * threadIdx.x; s < b16; s += 16u * kQtBlock)
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

// at most 256 * 16 workgroups (the test-only library: OEM_QUANT_GRID_BLOCKS, so that a few hundred lines take several
// rounds)
int quant_grid(uint64_t n)
{
    const long cap = knob("OEM_QUANT_GRID_BLOCKS", 256 * 16);
    const uint64_t g = (n + kQtBlock - 1) / kQtBlock;
    return (int)std::min<uint64_t>(std::max<uint64_t>(g, 1), (uint64_t)std::max(cap, 1L));
}

// -- the host side of the two descriptions: the caller's columns, the greatest length of a line, the upload ---------------
template <typename T>
int grow(T **p, uint64_t *cap, uint64_t n)
{
    if (n <= *cap && *p) return OEM_OK;
    (void)hipFree(*p); // (the lane is idle: its last chunk is finished)
    *p = nullptr;
    *cap = 0;
    OEM_TRY(dev_alloc(p, n, nullptr));
    *cap = n;
    return OEM_OK;
}

struct QuantSource {
    const uint8_t *names;
    const uint64_t *name_off;
    const uint64_t *lens;
    const double *counts;
    using Lines = QuantLines;
    struct Bufs {
        uint8_t *names = nullptr;
        uint64_t *name_off = nullptr, *lens = nullptr, *counts = nullptr;
        uint64_t names_cap = 0, lines_cap = 0, off_cap = 0, counts_cap = 0;
        ~Bufs()
        {
            (void)hipFree(names);
            (void)hipFree(name_off);
            (void)hipFree(lens);
            (void)hipFree(counts);
        }
    };
    uint64_t bound(uint64_t i) const { return (name_off[i + 1] - name_off[i]) + QuantLines::kMaxTail; }
    int upload(Bufs &b, uint64_t i0, uint64_t i1, hipStream_t st, Lines *view) const
    {
        const uint64_t n = i1 - i0, nb = name_off[i1] - name_off[i0];
        OEM_TRY(grow(&b.names, &b.names_cap, nb));
        OEM_TRY(grow(&b.name_off, &b.off_cap, n + 1));
        OEM_TRY(grow(&b.lens, &b.lines_cap, n));
        OEM_TRY(grow(&b.counts, &b.counts_cap, n));
        if (nb) OEM_HIP(hipMemcpyAsync(b.names, names + name_off[i0], nb, hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(b.name_off, name_off + i0, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(b.lens, lens + i0, sizeof(uint64_t) * n, hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(b.counts, counts + i0, sizeof(double) * n, hipMemcpyHostToDevice, st));
        *view = Lines{b.names, b.name_off, b.lens, b.counts};
        return OEM_OK;
    }
};

struct AmbigSource {
    const uint32_t *unique;
    const uint32_t *total;
    using Lines = AmbigLines;
    struct Bufs {
        uint32_t *unique = nullptr, *total = nullptr;
        uint64_t u_cap = 0, t_cap = 0;
        ~Bufs()
        {
            (void)hipFree(unique);
            (void)hipFree(total);
        }
    };
    uint64_t bound(uint64_t) const { return AmbigLines::kMaxLine; }
    int upload(Bufs &b, uint64_t i0, uint64_t i1, hipStream_t st, Lines *view) const
    {
        const uint64_t n = i1 - i0;
        OEM_TRY(grow(&b.unique, &b.u_cap, n));
        OEM_TRY(grow(&b.total, &b.t_cap, n));
        OEM_HIP(hipMemcpyAsync(b.unique, unique + i0, sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
        OEM_HIP(hipMemcpyAsync(b.total, total + i0, sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
        *view = Lines{b.unique, b.total};
        return OEM_OK;
    }
};

// One of the two lanes: a stream, the buffers of the chunk that runs on it, and that chunk while it is in flight.
template <class Src>
struct LinesLane {
    hipStream_t stream = nullptr;
    typename Src::Bufs in;
    uint64_t *len = nullptr, *off = nullptr;
    uint8_t *text = nullptr, *tmp = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // before measure, after it, after the scan, after emit
    bool busy = false;
    uint64_t i0 = 0, i1 = 0;
    LinesLane() = default;
    LinesLane(const LinesLane &) = delete;
    LinesLane &operator=(const LinesLane &) = delete;
    ~LinesLane()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        (void)hipFree(len);
        (void)hipFree(off);
        (void)hipFree(text);
        (void)hipFree(tmp);
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// The text of the n lines of `src` after the prefix.
template <class Src>
int lines_text(const Src &src, uint64_t n, const uint8_t *prefix, uint64_t prefix_len, oem_text_result *res)
{
    res->n_lines = res->n_kept = n;
    res->line_off.assign(n + 1, 0);
    res->kept.assign(n, 1u);
    double info[6] = {0, 0, 0, 0, 0, 0};
    if (n == 0) {
        res->n_bytes = prefix_len;
        res->text.reset(new uint8_t[prefix_len ? prefix_len : 1]);
        if (prefix_len) std::memcpy(res->text.get(), prefix, prefix_len);
        std::memcpy(g_quant_last, info, sizeof info);
        return OEM_OK;
    }
    const bool timing = knob("OEM_QUANT_TIMING", 0) != 0;
    const long cap_knob = knob("OEM_QUANT_BUF_BYTES", (long)kQtBufBytes);
    const uint64_t cap = cap_knob > 0 ? (uint64_t)cap_knob : kQtBufBytes;
    // The chunks: consecutive lines whose greatest lengths together fit the text buffer (one line at the least: a
    // line longer than the buffer gets a buffer of its own size).  cuts[c] .. cuts[c + 1] are the lines of chunk c.
    std::vector<uint64_t> cuts{0};
    uint64_t max_lines = 0, max_bytes = 0;
    {
        uint64_t acc = 0, start = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t b = src.bound(i);
            if (i > start && (acc + b > cap || i - start == kQtMaxChunk)) {
                cuts.push_back(i);
                start = i;
                acc = 0;
            }
            acc += b;
            max_bytes = std::max(max_bytes, acc);
            max_lines = std::max(max_lines, i + 1 - start);
        }
        cuts.push_back(n);
    }
    const size_t n_chunks = cuts.size() - 1;
    // the body starts at byte prefix_len of the file: the text buffers hold it from that position's residue modulo 16
    // on, so the kernel's aligned 16-byte words are aligned words of the file's first chunk as well
    const uint32_t shift0 = (uint32_t)(prefix_len & 15u);

    LinesLane<Src> lanes[2];
    size_t tmp_bytes = 0;
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)(max_lines + 1),
                                             (hipStream_t) nullptr));
    for (auto &ln : lanes) {
        OEM_HIP(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
        OEM_TRY(dev_alloc(&ln.len, max_lines + 1, nullptr));
        OEM_TRY(dev_alloc(&ln.off, max_lines + 1, nullptr));
        OEM_TRY(dev_alloc(&ln.text, max_bytes + 16, nullptr));
        OEM_TRY(dev_alloc(&ln.tmp, tmp_bytes, nullptr));
        if (timing)
            for (auto &e : ln.ev) OEM_HIP(hipEventCreate(&e));
        if (n_chunks == 1) break; // one chunk: one lane
    }

    // The host text.  Its size is known only when the last chunk is measured, so it is sized from the lines measured so
    // far (their mean length for the lines still to come, and a sixteenth more) and grows if that falls short.
    uint64_t text_cap = 0;
    auto reserve_text = [&](uint64_t done, uint64_t body_bytes, uint64_t body_have) -> int {
        const uint64_t need = prefix_len + body_bytes;
        if (need <= text_cap) return OEM_OK;
        const uint64_t mean = (body_bytes + done - 1) / done;
        const uint64_t rest = (n - done) * mean;
        const uint64_t want = need + rest + rest / 16 + (done < n ? 4096 : 0);
        for (auto &ln : lanes) // the copies into the text so far
            if (ln.stream) OEM_HIP(hipStreamSynchronize(ln.stream));
        std::unique_ptr<uint8_t[]> grown(new uint8_t[want]);
        if (res->text) std::memcpy(grown.get(), res->text.get(), prefix_len + body_have);
        else if (prefix_len) std::memcpy(grown.get(), prefix, prefix_len);
        res->text = std::move(grown);
        text_cap = want;
        return OEM_OK;
    };

    // the chunk in flight on a lane: its offsets have arrived once its stream is idle; they place its text
    auto finish = [&](LinesLane<Src> &ln) -> int {
        if (!ln.busy) return OEM_OK;
        ln.busy = false;
        OEM_HIP(hipStreamSynchronize(ln.stream));
        uint64_t *lo = res->line_off.data();
        const uint64_t base = lo[ln.i0]; // (the chunk before this one is finished: final)
        // the tiles of the chunk as k_lines_emit cut them: which of them fitted the stage
        for (uint64_t f = ln.i0; f < ln.i1; f += kQtBlock) {
            const uint64_t l = std::min<uint64_t>(f + kQtBlock, ln.i1);
            const uint64_t tile_bytes = lo[l] - (f == ln.i0 ? 0 : lo[f]);
            info[tile_bytes > kQtStageLines ? 2 : 1] += 1;
        }
        for (uint64_t i = ln.i0 + 1; i <= ln.i1; ++i) lo[i] += base;
        OEM_TRY(reserve_text(ln.i1, lo[ln.i1], base));
        const uint64_t bytes = lo[ln.i1] - base;
        if (bytes)
            OEM_HIP(hipMemcpyAsync(res->text.get() + prefix_len + base, ln.text + shift0, bytes, hipMemcpyDeviceToHost, ln.stream));
        if (timing) {
            for (int k = 0; k < 3; ++k) {
                float t = 0.f;
                OEM_HIP(hipEventElapsedTime(&t, ln.ev[k], ln.ev[k + 1]));
                info[3 + k] += t;
            }
        }
        return OEM_OK;
    };

    for (size_t c = 0; c < n_chunks; ++c) {
        const uint64_t i0 = cuts[c], i1 = cuts[c + 1];
        const uint32_t m = (uint32_t)(i1 - i0);
        LinesLane<Src> &ln = lanes[c & 1];
        typename Src::Lines view;
        OEM_TRY(src.upload(ln.in, i0, i1, ln.stream, &view));
        OEM_HIP(hipMemsetAsync(ln.len + m, 0, sizeof(uint64_t), ln.stream));
        if (timing) OEM_HIP(hipEventRecord(ln.ev[0], ln.stream));
        hipLaunchKernelGGL(k_lines_measure<typename Src::Lines>, dim3(quant_grid(m)), dim3(kQtBlock), 0, ln.stream, view, m, ln.len);
        OEM_HIP(hipGetLastError());
        if (timing) OEM_HIP(hipEventRecord(ln.ev[1], ln.stream));
        {
            size_t tb = tmp_bytes;
            OEM_HIP(hipcub::DeviceScan::ExclusiveSum(ln.tmp, tb, (const uint64_t *)ln.len, ln.off, (int)(m + 1), ln.stream));
        }
        if (timing) OEM_HIP(hipEventRecord(ln.ev[2], ln.stream));
        hipLaunchKernelGGL(k_lines_emit<typename Src::Lines>, dim3(quant_grid(m)), dim3(kQtBlock), 0, ln.stream, view,
                           (const uint64_t *)ln.off, m, ln.text + shift0);
        OEM_HIP(hipGetLastError());
        if (timing) OEM_HIP(hipEventRecord(ln.ev[3], ln.stream));
        // the ends of the chunk's lines, relative to the chunk (finish() makes them offsets into the body)
        OEM_HIP(hipMemcpyAsync(res->line_off.data() + i0 + 1, ln.off + 1, sizeof(uint64_t) * m, hipMemcpyDeviceToHost, ln.stream));
        ln.busy = true;
        ln.i0 = i0;
        ln.i1 = i1;
        // the previous chunk's text comes back while this chunk's kernels run
        OEM_TRY(finish(lanes[(c & 1) ^ 1]));
    }
    OEM_TRY(finish(lanes[0])); // (one of the two is in flight: the last chunk)
    OEM_TRY(finish(lanes[1]));
    for (auto &ln : lanes)
        if (ln.stream) OEM_HIP(hipStreamSynchronize(ln.stream));
    res->n_bytes = prefix_len + res->line_off[n];
    info[0] = (double)n_chunks;
    std::memcpy(g_quant_last, info, sizeof info);
    return OEM_OK;
}

template <class Src>
int lines_text_call(const Src &src, uint64_t n, const uint8_t *prefix, uint64_t prefix_len, int device, oem_text_result **out)
{
    OEM_TRY(ensure_device(device));
    std::unique_ptr<oem_text_result> res(new oem_text_result);
    OEM_TRY(lines_text(src, n, prefix, prefix_len, res.get()));
    res->content_bytes = res->n_bytes;
    *out = res.release();
    return OEM_OK;
}

} // namespace

void quant_last_call(double *out6) { std::memcpy(out6, g_quant_last, sizeof g_quant_last); }

} // namespace oem

using namespace oem;

extern "C" int oem_quant_text(const uint8_t *names, const uint64_t *name_off, const uint64_t *lens, const double *counts,
                              uint32_t n_txps, const uint8_t *prefix, uint64_t prefix_len, int device, oem_text_result **out)
{
    OEM_API_BEGIN
    if (out) *out = nullptr;
    if (!out) return fail(OEM_ERR_ARG, "oem_quant_text: out is NULL");
    if (!prefix && prefix_len) return fail(OEM_ERR_ARG, "oem_quant_text: prefix is NULL and prefix_len is not 0");
    if (n_txps && (!names || !name_off || !lens || !counts))
        return fail(OEM_ERR_ARG, "oem_quant_text: names, name_off, lens or counts is NULL and n_txps is not 0");
    for (uint32_t t = 0; t < n_txps; ++t) {
        if (name_off[t + 1] < name_off[t]) return fail(OEM_ERR_ARG, "oem_quant_text: name_off must be non-decreasing (transcript %u)", t);
        const uint8_t *p = names + name_off[t];
        const uint64_t nl = name_off[t + 1] - name_off[t];
        if (nl && (std::memchr(p, '\t', nl) || std::memchr(p, '\n', nl)))
            return fail(OEM_ERR_ARG, "oem_quant_text: the name of transcript %u contains a tab or a newline", t);
        if (!f64_is_finite(f64_bits(counts[t]))) return fail(OEM_ERR_ARG, "oem_quant_text: counts[%u] is not finite", t);
    }
    const QuantSource src{names, name_off, lens, counts};
    return lines_text_call(src, n_txps, prefix, prefix_len, device, out);
    OEM_API_END("oem_quant_text")
}

extern "C" int oem_ambig_text(const uint32_t *unique, const uint32_t *total, uint32_t n_txps, const uint8_t *prefix,
                              uint64_t prefix_len, int device, oem_text_result **out)
{
    OEM_API_BEGIN
    if (out) *out = nullptr;
    if (!out) return fail(OEM_ERR_ARG, "oem_ambig_text: out is NULL");
    if (!prefix && prefix_len) return fail(OEM_ERR_ARG, "oem_ambig_text: prefix is NULL and prefix_len is not 0");
    if (n_txps && (!unique || !total)) return fail(OEM_ERR_ARG, "oem_ambig_text: unique or total is NULL and n_txps is not 0");
    const AmbigSource src{unique, total};
    return lines_text_call(src, n_txps, prefix, prefix_len, device, out);
    OEM_API_END("oem_ambig_text")
}
