// oem_lz4.hip -- LZ4 blocks of a device byte range, compressed on the device (oem_assignment_text_lz4).
//
// The range is cut into independent blocks of at most 64 KiB (oem_lz4.h: the frame's BD), so every match offset fits
// the format's 16 bits by construction.  Three steps on the caller's stream:
//   k_lz4_blocks   one wavefront per block: a greedy parse, 64 positions at a time.  The block's payload goes to its
//                  bound-strided slot, its size and the XXH32 of the payload as stored to two arrays.  A block that
//                  does not shrink is kept raw: its payload stays where it is, in the input.
//   (hipcub scan)  4 + size + 4 per block -> the blocks' offsets in the frame, and the length of the chunk's frame
//   k_lz4_gather   size word (high bit set on a raw block), payload and checksum copied into place
//
// The parse.  A window is the 64 positions from the cursor on.  Every lane hashes the 4 bytes at its position, reads its
// candidate from the wave's table (4096 u16 positions in LDS, zero at the start: position 0 is a legal candidate and is
// verified like any other), and verifies it (cand < p, 4 equal bytes).  All lanes read before any lane writes, so the
// candidates of a window come from before the window: two positions of one window never match each other.  The first
// lane with a match wins; the match is extended forward 64 bytes at a time (the source may overlap itself: the
// compare reads the input, offsets 1 .. 3 included) up to the last 5 bytes.  The window's positions up to the match
// and the positions inside the match are inserted, and the cursor moves to the match's end.  Where lanes of one
// insertion hash to the same slot the highest position is stored: a lane writes only while its position exceeds what
// the slot holds, and the wave repeats until no lane has anything to write.  So the table, and with it the output, is
// a function of the input bytes alone, whatever order the LDS serves the lanes in.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>

#include "oem_driver.h"
#include "oem_lz4.h"

namespace oem {
namespace {

constexpr uint32_t kHashBits = 12;
constexpr uint32_t kTableSize = 1u << kHashBits;
constexpr int kGatherBlock = 256;

__device__ __forceinline__ uint32_t load4(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// The wave's table, addressed as LDS (a generic pointer would make every volatile access a flat one).  Volatile: a lane
// must see what OTHER lanes of its wave stored, so the compiler may neither forward a lane's own store to its next
// load nor reorder the accesses.
typedef __attribute__((address_space(3))) volatile uint16_t TableSlot;

__device__ __forceinline__ uint32_t first_lane(unsigned long long mask) { return (uint32_t)__ffsll((long long)mask) - 1u; }

// table[h] = max(table[h], p) over the lanes with `on`, by rule (see the top of the file)
__device__ __forceinline__ void table_insert(TableSlot *table, uint32_t h, uint32_t p, bool on)
{
    for (;;) {
        const bool need = on && p > (uint32_t)table[h];
        if (!__ballot(need)) break;
        if (need) table[h] = (uint16_t)p;
        __builtin_amdgcn_wave_barrier();
    }
}

// One sequence at dst, by the whole wave: seq_layout() says where the parts go, seq_head_byte / seq_tail_byte what they
// hold.  match_len == 0: the last literals.  Returns its length.
__device__ __forceinline__ uint32_t wave_emit_sequence(uint8_t *__restrict__ dst, const uint8_t *__restrict__ lit, uint32_t lit_len,
                                                       uint32_t offset, uint32_t match_len, uint32_t lane)
{
    const lz4::SeqLayout l = lz4::seq_layout(lit_len, match_len);
    for (uint32_t i = lane; i < l.head; i += 64) dst[i] = lz4::seq_head_byte(lit_len, match_len, i);
    for (uint32_t i = lane; i < lit_len; i += 64) dst[l.head + i] = lit[i];
    for (uint32_t i = lane; i < l.tail; i += 64) dst[l.head + lit_len + i] = lz4::seq_tail_byte(offset, match_len, i);
    return l.total;
}

// One wavefront per block.  sizes[b] = bytes of the payload as stored (== the block's length: raw, the payload is the
// input), sums[b] = its XXH32.
__global__ __launch_bounds__(64) void k_lz4_blocks(const uint8_t *__restrict__ in, uint64_t n_bytes, uint32_t block_bytes,
                                                   uint64_t slot_stride, uint8_t *__restrict__ slots,
                                                   uint32_t *__restrict__ sizes, uint32_t *__restrict__ sums)
{
    __shared__ uint16_t table_mem[kTableSize];
    TableSlot *table = (TableSlot *)table_mem;
    const uint32_t lane = threadIdx.x;
    const uint64_t b = blockIdx.x;
    const uint64_t begin = b * block_bytes;
    const uint8_t *__restrict__ src = in + begin;
    const uint32_t n = n_bytes - begin < block_bytes ? (uint32_t)(n_bytes - begin) : block_bytes;
    uint8_t *dst = slots + b * slot_stride;

    for (uint32_t i = lane; i < kTableSize; i += 64) table[i] = 0;
    __builtin_amdgcn_wave_barrier();

    uint32_t pos = 0, anchor = 0, op = 0; // the same in every lane
    if (n >= lz4::kMinMatchBlock) {
        const uint32_t match_limit = n - lz4::kMatchFreeTail; // a match starts below it
        const uint32_t match_end = n - lz4::kLastLiterals;    // and ends at or below it
        while (pos < match_limit) {
            const uint32_t p = pos + lane;
            const bool valid = p < match_limit;
            uint32_t v = 0, h = 0, cand = 0;
            bool ok = false;
            if (valid) {
                v = load4(src + p);
                h = lz4::hash4(v, kHashBits);
                cand = table[h];
                ok = cand < p && load4(src + cand) == v;
            }
            __builtin_amdgcn_wave_barrier();
            const unsigned long long found = __ballot(ok);
            if (!found) {
                table_insert(table, h, p, valid);
                pos += 64;
                continue;
            }
            const uint32_t first = first_lane(found);
            const uint32_t mp = pos + first;
            const uint32_t offset = mp - (uint32_t)__builtin_amdgcn_readlane((int)cand, (int)first);
            uint32_t len = lz4::kMinMatch; // mp + 4 <= n - 9: inside match_end
            for (;;) {
                const uint32_t i = mp + len + lane;
                const bool same = i < match_end && src[i] == src[i - offset];
                const unsigned long long stop = __ballot(!same);
                if (stop) {
                    len += first_lane(stop);
                    break;
                }
                len += 64;
            }
            op += wave_emit_sequence(dst + op, src + anchor, mp - anchor, offset, len, lane);
            // the window's positions up to the match, then the positions inside it
            table_insert(table, h, p, valid && lane <= first);
            const uint32_t ins_end = mp + len < match_limit ? mp + len : match_limit;
            for (uint32_t q = mp + 1; q < ins_end; q += 64) {
                const uint32_t p2 = q + lane;
                const bool on = p2 < ins_end;
                const uint32_t h2 = on ? lz4::hash4(load4(src + p2), kHashBits) : 0u;
                table_insert(table, h2, p2, on);
            }
            pos = anchor = mp + len;
        }
    }
    op += wave_emit_sequence(dst + op, src + anchor, n - anchor, 0, 0, lane);

    // the payload as stored, and its checksum: lanes 0 .. 3 each run one accumulator over the 16-byte stripes
    const bool raw = op >= n;
    const uint8_t *payload = raw ? src : dst;
    const uint32_t size = raw ? n : op;
    __threadfence(); // the slot's bytes, written by other lanes of this wave, are read below
    uint32_t acc = lz4::xxh32_acc_init(lane & 3u, 0);
    if (lane < 4) {
        const uint32_t stripes = size / 16;
        for (uint32_t s = 0; s < stripes; ++s) acc = lz4::xxh32_round(acc, load4(payload + 16 * s + 4 * lane));
    }
    const uint32_t v0 = __shfl(acc, 0), v1 = __shfl(acc, 1), v2 = __shfl(acc, 2), v3 = __shfl(acc, 3);
    if (lane == 0) {
        sizes[b] = size;
        sums[b] = lz4::xxh32_finish(v0, v1, v2, v3, payload + (size & ~15u), size, 0);
    }
}

struct BlockFrameBytes {
    __host__ __device__ uint64_t operator()(uint32_t size) const { return (uint64_t)size + lz4::kBlockOverheadBytes; }
};

// One workgroup per block: size word, payload, checksum at frame + offs[b].  A block whose stored size is its own
// length was kept raw: its payload comes from the input and its size word gets the high bit.
__global__ __launch_bounds__(kGatherBlock) void k_lz4_gather(const uint8_t *__restrict__ in, uint64_t n_bytes, uint32_t block_bytes,
                                                             uint64_t slot_stride, const uint8_t *__restrict__ slots,
                                                             const uint32_t *__restrict__ sizes, const uint32_t *__restrict__ sums,
                                                             const uint64_t *__restrict__ offs, uint8_t *__restrict__ frame,
                                                             unsigned long long *__restrict__ raw_blocks)
{
    const uint64_t b = blockIdx.x;
    const uint32_t t = threadIdx.x;
    const uint64_t begin = b * block_bytes;
    const uint32_t n = n_bytes - begin < block_bytes ? (uint32_t)(n_bytes - begin) : block_bytes;
    const uint32_t size = sizes[b];
    const bool raw = size == n;
    const uint8_t *__restrict__ src = raw ? in + begin : slots + b * slot_stride;
    uint8_t *__restrict__ dst = frame + offs[b];
    if (t < 4) {
        dst[t] = (uint8_t)((size | (raw ? lz4::kBlockRawBit : 0u)) >> (8 * t));
        dst[4 + size + t] = (uint8_t)(sums[b] >> (8 * t));
    }
    for (uint32_t i = t; i < size; i += kGatherBlock) dst[4 + i] = src[i];
    if (t == 0 && raw) atomicAdd(raw_blocks, 1ull);
}

// a device buffer of at least `need` elements; the stream is idle when it is replaced
template <typename T>
int chunk_reserve(hipStream_t st, T **buf, uint64_t *cap, uint64_t need)
{
    if (need <= *cap && *buf) return OEM_OK;
    OEM_HIP(hipStreamSynchronize(st));
    (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    OEM_TRY(dev_alloc(buf, (size_t)need, nullptr));
    *cap = need;
    return OEM_OK;
}

} // namespace

Lz4Chunk::~Lz4Chunk()
{
    (void)hipFree(slots);
    (void)hipFree(sizes);
    (void)hipFree(sums);
    (void)hipFree(offs);
    (void)hipFree(tmp);
    (void)hipFree(frame);
    (void)hipFree(d_raw);
    if (h_info) (void)hipHostFree(h_info);
}

uint32_t lz4_block_bytes()
{
    const long v = knob("OEM_LZ4_BLOCK_BYTES", (long)lz4::kBlockMaxBytes);
    return (uint32_t)std::min<long>(std::max<long>(v, 1), (long)lz4::kBlockMaxBytes);
}

uint64_t lz4_blocks_of(uint64_t n, uint32_t block_bytes) { return (n + block_bytes - 1) / block_bytes; }

int lz4_chunk_enqueue(Lz4Chunk &c, const uint8_t *d_in, uint64_t n, uint32_t block_bytes, hipStream_t st, hipEvent_t ev_blocks,
                      hipEvent_t ev_gather)
{
    const uint64_t nb = lz4_blocks_of(n, block_bytes);
    if (nb > 0x7ffffffeull) return fail(OEM_ERR_STATE, "lz4: %llu blocks in one chunk", (unsigned long long)nb);
    c.n_blocks = nb;
    if (!c.h_info) OEM_HIP(hipHostMalloc((void **)&c.h_info, 2 * sizeof(uint64_t), hipHostMallocDefault));
    if (!c.d_raw) OEM_TRY(dev_alloc(&c.d_raw, 1, nullptr));
    c.h_info[0] = c.h_info[1] = 0;
    if (nb == 0) return OEM_OK;
    const uint64_t stride = ((uint64_t)lz4::block_bound(block_bytes) + 15u) & ~(uint64_t)15u;
    OEM_TRY(chunk_reserve(st, &c.slots, &c.slots_cap, nb * stride));
    uint64_t cap = c.blocks_cap;
    OEM_TRY(chunk_reserve(st, &c.sizes, &cap, nb + 1));
    cap = c.blocks_cap;
    OEM_TRY(chunk_reserve(st, &c.sums, &cap, nb + 1));
    OEM_TRY(chunk_reserve(st, &c.offs, &c.blocks_cap, nb + 1));
    OEM_TRY(chunk_reserve(st, &c.frame, &c.frame_cap, n + lz4::kBlockOverheadBytes * nb));

    OEM_HIP(hipMemsetAsync(c.sizes + nb, 0, sizeof(uint32_t), st));
    OEM_HIP(hipMemsetAsync(c.d_raw, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_lz4_blocks, dim3((unsigned)nb), dim3(64), 0, st, d_in, n, block_bytes, stride, c.slots, c.sizes, c.sums);
    OEM_HIP(hipGetLastError());
    if (ev_blocks) OEM_HIP(hipEventRecord(ev_blocks, st));
    {
        hipcub::TransformInputIterator<uint64_t, BlockFrameBytes, const uint32_t *> it(c.sizes, BlockFrameBytes());
        size_t tmp_bytes = 0;
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, it, c.offs, (int)(nb + 1), st));
        OEM_TRY(chunk_reserve(st, &c.tmp, &c.tmp_cap, (uint64_t)tmp_bytes));
        OEM_HIP(hipcub::DeviceScan::ExclusiveSum(c.tmp, tmp_bytes, it, c.offs, (int)(nb + 1), st));
    }
    hipLaunchKernelGGL(k_lz4_gather, dim3((unsigned)nb), dim3(kGatherBlock), 0, st, d_in, n, block_bytes, stride, c.slots, c.sizes,
                       c.sums, c.offs, c.frame, c.d_raw);
    OEM_HIP(hipGetLastError());
    if (ev_gather) OEM_HIP(hipEventRecord(ev_gather, st));
    // the host learns the chunk's frame length (and its raw blocks) from here
    OEM_HIP(hipMemcpyAsync(c.h_info, c.offs + nb, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    OEM_HIP(hipMemcpyAsync(c.h_info + 1, c.d_raw, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    return OEM_OK;
}

int lz4_frame_from_host(const uint8_t *data, uint64_t n, hipStream_t st, std::unique_ptr<uint8_t[]> *out, uint64_t *out_len,
                        uint64_t *n_blocks, uint64_t *raw_blocks)
{
    const uint32_t bb = lz4_block_bytes();
    const uint64_t nb = lz4_blocks_of(n, bb);
    out->reset(new uint8_t[lz4::kFrameHeaderBytes + n + lz4::kBlockOverheadBytes * nb + lz4::kEndMarkBytes]);
    uint8_t *f = out->get();
    lz4::frame_header(f, n);
    uint64_t at = lz4::kFrameHeaderBytes;
    *n_blocks = nb;
    *raw_blocks = 0;
    if (n) {
        DevBuf<uint8_t> d_in;
        Lz4Chunk c;
        OEM_TRY(dev_alloc(&d_in.p, (size_t)n, nullptr));
        OEM_HIP(hipMemcpyAsync(d_in.p, data, n, hipMemcpyHostToDevice, st));
        int rc = lz4_chunk_enqueue(c, d_in.p, n, bb, st);
        hipError_t e = hipStreamSynchronize(st); // before the buffers go, whatever happened
        OEM_TRY(rc);
        OEM_HIP(e);
        OEM_HIP(hipMemcpy(f + at, c.frame, c.h_info[0], hipMemcpyDeviceToHost));
        at += c.h_info[0];
        *raw_blocks = c.h_info[1];
    }
    std::memset(f + at, 0, lz4::kEndMarkBytes);
    *out_len = at + lz4::kEndMarkBytes;
    return OEM_OK;
}

} // namespace oem
