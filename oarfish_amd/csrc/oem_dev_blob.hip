// oem_dev_blob.hip -- DevBlob and SurvivorArena (oem_dev_blob.h): the growth, the append and the move of a tail, with
// their two kernels.
#include "oem_dev_blob.h"
#include "oem_filter_device.h"

namespace oem {
namespace {

constexpr int kDT = 256;
inline dim3 grid_of(uint64_t n) { return dim3((unsigned)std::max<uint64_t>((n + kDT - 1) / kDT, 1)); }

// dst[k] = src[k] + add over cnt offsets: a batch's dense offsets rebased to the blob's bytes, or (add wraps) a tail's
// offsets moved down by its first byte
__global__ __launch_bounds__(kDT) void k_offsets_rebase(uint64_t cnt, const uint64_t *__restrict__ src, uint64_t add, uint64_t *__restrict__ dst)
{
    const uint64_t k = (uint64_t)blockIdx.x * kDT + threadIdx.x;
    if (k < cnt) dst[k] = src[k] + add;
}

// The per-survivor words of an append, one lane per survivor k < m of the batch, which becomes arena record base + k
// (below cap: reserved by the caller, and checked here):
//   gidx[base + k] = rec_base + order[k], its session-global input index (order[k] < n_in, the batch's size)
//   sec[base + k]  = src_sec[k] != 0, or 0 for a batch without flags
__global__ __launch_bounds__(kDT) void k_survivor_append(uint64_t m, uint64_t n_in, uint64_t base, uint64_t cap, uint64_t rec_base,
                                                         const uint32_t *__restrict__ order, const uint8_t *__restrict__ src_sec,
                                                         uint64_t *__restrict__ gidx, uint8_t *__restrict__ sec)
{
    const uint64_t k = (uint64_t)blockIdx.x * kDT + threadIdx.x;
    if (k >= m || base + k >= cap) return;
    const uint32_t i = order[k];
    gidx[base + k] = i < n_in ? rec_base + i : kNoRecord;
    sec[base + k] = src_sec ? (uint8_t)(src_sec[k] != 0) : (uint8_t)0;
}

// b at `count` elements with its first `used` copied over; the previous allocation goes to *old
template <typename T>
int regrow(DevBuf<T> *b, uint64_t used, uint64_t count, DevBuf<T> *old)
{
    DevBuf<T> grown;
    OEM_TRY(dev_alloc(&grown.p, count, nullptr));
    if (used) OEM_HIP(hipMemcpy(grown.p, b->p, sizeof(T) * used, hipMemcpyDeviceToDevice));
    std::swap(b->p, grown.p);
    std::swap(old->p, grown.p);
    return OEM_OK;
}

// an instance's floor as next_cap takes it (the testing library: the knob replaces every instance's)
uint64_t floor_of(const char *knob_name, uint64_t first) { return (uint64_t)std::max<long>(knob(knob_name, (long)first), 1); }

} // namespace

int DevBlob::grow_entries(uint64_t to, DevBuf<uint64_t> *old)
{
    const bool fresh = !off.p;
    OEM_TRY(regrow(&off, fresh ? 0 : n + 1, blob_alloc_offsets(to), old));
    if (fresh) OEM_HIP(hipMemset(off.p, 0, sizeof(uint64_t)));
    cap = to;
    return OEM_OK;
}

int DevBlob::grow_bytes(uint64_t to, DevBuf<uint8_t> *old)
{
    OEM_TRY(regrow(&bytes, n_bytes, blob_alloc_bytes(to), old));
    OEM_HIP(hipMemset(bytes.p + n_bytes, 0, kBlobPad));
    cap_bytes = to;
    return OEM_OK;
}

int DevBlob::reserve(uint64_t n_need, uint64_t bytes_need, uint64_t first_n, uint64_t first_bytes, uint64_t others, uint64_t *peak)
{
    if (n_need > cap || !off.p) {
        const uint64_t to = next_cap(cap, n_need, floor_of("OEM_ARENA_RECORDS0", first_n));
        if (peak) *peak = std::max(*peak, others + held() + sizeof(uint64_t) * blob_alloc_offsets(to));
        DevBuf<uint64_t> old;
        OEM_TRY(grow_entries(to, &old));
    }
    if (bytes_need > cap_bytes || !bytes.p) {
        const uint64_t to = next_cap(cap_bytes, bytes_need, floor_of("OEM_ARENA_BYTES0", first_bytes));
        if (peak) *peak = std::max(*peak, others + held() + blob_alloc_bytes(to));
        DevBuf<uint8_t> old;
        OEM_TRY(grow_bytes(to, &old));
    }
    return OEM_OK;
}

// m items of nb bytes behind the n: their bytes, the padding, and their m offsets d_off[1 .. m] rebased by `add`
int DevBlob::put(const uint8_t *d_bytes, const uint64_t *d_off, uint64_t m, uint64_t nb, uint64_t add)
{
    if (n + m > cap || n_bytes + nb > cap_bytes) return fail(OEM_ERR_STATE, "DevBlob: no room was reserved for %llu items", (unsigned long long)m);
    if (nb) OEM_HIP(hipMemcpyAsync(bytes.p + n_bytes, d_bytes, nb, hipMemcpyDeviceToDevice, nullptr));
    OEM_HIP(hipMemsetAsync(bytes.p + n_bytes + nb, 0, kBlobPad, nullptr));
    hipLaunchKernelGGL(k_offsets_rebase, grid_of(m), dim3(kDT), 0, nullptr, m, d_off + 1, add, off.p + n + 1);
    OEM_HIP(hipGetLastError());
    n += m;
    n_bytes += nb;
    return OEM_OK;
}

int DevBlob::move_tail(const DevBlob &src, uint64_t first_entry, uint64_t first_byte)
{
    if (n || first_entry > src.n || first_byte > src.n_bytes) return fail(OEM_ERR_STATE, "DevBlob::move_tail: not a tail for an empty blob");
    return put(src.bytes.p + first_byte, src.off.p + first_entry, src.n - first_entry, src.n_bytes - first_byte, (uint64_t)0 - first_byte);
}

// Every array that shares the capacity grows in one step: all of them are alive twice until it is over.
int SurvivorArena::grow_entries(uint64_t to)
{
    peak = std::max(peak, held() + own_bytes(to) + sizeof(uint64_t) * blob_alloc_offsets(to) * (with_umis ? 2 : 1));
    DevBuf<oem_aln_record> r0;
    DevBuf<uint64_t> g0, no0, uo0;
    DevBuf<uint8_t> s0;
    DevBuf<uint32_t> c0;
    OEM_TRY(regrow(&rec, n, to, &r0));
    OEM_TRY(regrow(&gidx, n, to, &g0));
    OEM_TRY(regrow(&sec, n, flags_alloc_bytes(to), &s0));
    OEM_HIP(hipMemset(sec.p + n, 0, kFlagPad));
    if (with_ids) OEM_TRY(regrow(&cell_id, n, to, &c0));
    OEM_TRY(names.grow_entries(to, &no0));
    if (with_umis) OEM_TRY(umis.grow_entries(to, &uo0));
    cap = to;
    return OEM_OK;
}

int SurvivorArena::reserve(uint64_t n_need, uint64_t name_bytes_need, uint64_t umi_bytes_need)
{
    if (n_need > cap || !rec.p) OEM_TRY(grow_entries(next_cap(cap, n_need, floor_of("OEM_ARENA_RECORDS0", first_n))));
    OEM_TRY(names.reserve(n_need, name_bytes_need, first_n, first_bytes, held() - names.held(), &peak)); // (the entries have grown above)
    if (with_umis) OEM_TRY(umis.reserve(n_need, umi_bytes_need, first_n, first_bytes, held() - umis.held(), &peak));
    return OEM_OK;
}

int SurvivorArena::make(uint64_t records, uint64_t name_bytes, uint64_t umi_bytes)
{
    DevBuf<uint8_t> none;
    OEM_TRY(grow_entries(records));
    OEM_TRY(names.grow_bytes(name_bytes, &none));
    if (with_umis) OEM_TRY(umis.grow_bytes(umi_bytes, &none));
    peak = held();
    return OEM_OK;
}

int SurvivorArena::append(uint64_t m, const uint32_t *d_order, const oem_aln_record *d_in, uint64_t n_in, uint64_t rec_base,
                          const uint8_t *d_names, const uint64_t *d_name_off, uint64_t name_bytes, const uint8_t *d_sec,
                          const uint32_t *d_cell_id, const uint8_t *d_umis, const uint64_t *d_umi_off, uint64_t umi_bytes)
{
    OEM_TRY(reserve(n + m, names.n_bytes + name_bytes, umis.n_bytes + umi_bytes));
    OEM_TRY(records_gather(m, d_order, d_in, rec.p + n));
    hipLaunchKernelGGL(k_survivor_append, grid_of(m), dim3(kDT), 0, nullptr, m, n_in, n, cap, rec_base, d_order, d_sec, gidx.p, sec.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemsetAsync(sec.p + n + m, 0, kFlagPad, nullptr));
    if (with_ids) OEM_HIP(hipMemcpyAsync(cell_id.p + n, d_cell_id, sizeof(uint32_t) * m, hipMemcpyDeviceToDevice, nullptr));
    OEM_TRY(names.append(d_names, d_name_off, m, name_bytes));
    if (with_umis) OEM_TRY(umis.append(d_umis, d_umi_off, m, umi_bytes));
    OEM_HIP(hipStreamSynchronize(nullptr));
    n += m;
    return OEM_OK;
}

int SurvivorArena::take_tail(const SurvivorArena &old, uint64_t t, uint64_t first_name_byte, uint64_t first_umi_byte)
{
    if (n || with_ids || t > old.n || old.n - t > cap) return fail(OEM_ERR_STATE, "SurvivorArena::take_tail: the tail does not fit an empty arena");
    const uint64_t tail = old.n - t;
    if (tail) { // (a collated session's: no cell ids)
        OEM_HIP(hipMemcpyAsync(rec.p, old.rec.p + t, sizeof(oem_aln_record) * tail, hipMemcpyDeviceToDevice, nullptr));
        OEM_HIP(hipMemcpyAsync(gidx.p, old.gidx.p + t, sizeof(uint64_t) * tail, hipMemcpyDeviceToDevice, nullptr));
        OEM_HIP(hipMemcpyAsync(sec.p, old.sec.p + t, tail, hipMemcpyDeviceToDevice, nullptr));
    }
    OEM_HIP(hipMemsetAsync(sec.p + tail, 0, kFlagPad, nullptr));
    OEM_TRY(names.move_tail(old.names, t, first_name_byte));
    if (with_umis) OEM_TRY(umis.move_tail(old.umis, t, first_umi_byte));
    OEM_HIP(hipStreamSynchronize(nullptr));
    n = tail;
    return OEM_OK;
}

} // namespace oem
