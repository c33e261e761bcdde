// oem_cells_barcodes_sort_stream.hip -- the any-order form of the barcoded cells session
// (oem_cells_stream_set_barcodes_any_order): the device side of oem_collate.h's "Cells from a stream in any order".
// Batches arrive through oem_cells_stream_push_barcodes as in the collated session (oem_cells_barcodes_stream.hip, which
// owns the staging, the parse worker and the arena); here is what differs:
//
//   per batch   the survivors' barcodes are INTERNED against the table of the labels seen so far (oem_barcode_table.h):
//               1. k_barcode_lookup, one survivor per lane, reads the table only: hash, probe, at an occupied slot the
//                  length and then the bytes 8 at a time against that label.  A hit gives cell_id[k]; EMPTY marks a miss.
//               2. the misses are compacted (scan + scatter), their barcodes gathered dense (gather_names) and collated
//                  as one cell (collate_barcodes_device: the key rounds of collate_resident, the runs' heads ranked by
//                  survivor index).  The new labels get the ids n_labels + rank and are appended to the label blob (a
//                  DevBlob, oem_dev_blob.h: the arena's blob, with its growth and its padding).
//               3. when the load would pass 1/2 a table of at least twice the capacity is built from the label blob;
//               4. k_barcode_insert, one label per lane, atomicCAS(slot, EMPTY, id) along the probe path (the keys are
//                  distinct by construction: nothing is compared);
//               5. the lookup again, over the misses only.
//               No kernel both reads and writes the table (the insert only claims free slots), no lane waits for another
//               lane's store, and every probe loop ends after `capacity` steps with an error word that the host turns
//               into a sticky OEM_ERR_STATE.  A survivor costs the arena 4 bytes of cell id, not its barcode.
//   NOTHING RUNS BEFORE FINISH: any barcode may come back in the last batch, so no cell is closed before it.
//   finish      a stable radix sort of (cell_id, position) over the bits n_cells needs gives order_bc; cell_rec_off is
//               the sorted keys' run starts; the labels come down once.  The session then lays its arena out in that
//               order and runs it as the collated session runs its cells.
#include <algorithm>
#include <cstring>
#include <mutex>

#include <hipcub/hipcub.hpp>

#include "oem_barcode_table.h"
#include "oem_cells_barcodes_stream.h"
#include "oem_collate_device.h"
#include "oem_parse_device.h"

namespace oem {
namespace {

constexpr int kIT = 256;
inline dim3 grid_of(uint64_t n) { return dim3((unsigned)std::max<uint64_t>((n + kIT - 1) / kIT, 1)); }
inline int bits_of(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

enum : int { kStatProbe = 0, kStatWrapped = 1, kStatError = 2, kStatWords = 3 };

// Survivor idx[j] (idx NULL: j) of the batch, j < cnt, against the table: cell_id[k] = its label's id, kBarcodeEmpty on a
// miss.  miss (or NULL): m + 1 flags for the scan, miss[m] = 0 (cnt == m, idx NULL).  must_hit: a miss is an error (the
// second pass, after the insert).  bc: the survivors' dense blob, padded by 16, with its offsets from 0.
__global__ __launch_bounds__(kIT) void k_barcode_lookup(uint64_t cnt, const uint32_t *__restrict__ idx, const uint8_t *__restrict__ bc,
                                                         const uint64_t *__restrict__ off, const uint32_t *__restrict__ slot, uint64_t capacity,
                                                         uint32_t hash_bits, const uint8_t *__restrict__ labels,
                                                         const uint64_t *__restrict__ label_off, uint64_t n_labels, uint32_t must_hit,
                                                         uint32_t *__restrict__ cell_id, uint32_t *__restrict__ miss,
                                                         unsigned long long *__restrict__ stats)
{
    const uint64_t j = (uint64_t)blockIdx.x * kIT + threadIdx.x;
    if (j > cnt) return;
    if (j == cnt) {
        if (miss) miss[cnt] = 0u;
        return;
    }
    const uint64_t k = idx ? idx[j] : j;
    const uint64_t b0 = off[k], len = off[k + 1] - b0;
    uint64_t steps = 0;
    bool wrapped = false;
    uint32_t id = barcode_table_find(slot, capacity, hash_bits, labels, label_off, bc + b0, len, &steps, &wrapped);
    if (steps > 1) atomicMax(stats + kStatProbe, (unsigned long long)steps);
    if (wrapped) atomicOr(stats + kStatWrapped, 1ull);
    if (id == kBarcodeProbeError || (id != kBarcodeEmpty && id >= n_labels) || (must_hit && id == kBarcodeEmpty)) {
        atomicOr(stats + kStatError, 1ull);
        id = kBarcodeEmpty;
    }
    cell_id[k] = id;
    if (miss) miss[k] = id == kBarcodeEmpty ? 1u : 0u;
}

// idx[at[k]] = k for the survivors that missed
__global__ __launch_bounds__(kIT) void k_barcode_miss_scatter(uint64_t m, const uint32_t *__restrict__ miss, const uint64_t *__restrict__ at,
                                                               uint32_t *__restrict__ idx)
{
    const uint64_t k = (uint64_t)blockIdx.x * kIT + threadIdx.x;
    if (k < m && miss[k]) idx[at[k]] = (uint32_t)k;
}

// Label first + j, j < cnt, into the first free slot of its probe path.  The labels are distinct, so nothing is compared:
// a lane claims a slot with one compare-and-swap or moves on, and never waits for another lane.
__global__ __launch_bounds__(kIT) void k_barcode_insert(uint64_t first, uint64_t cnt, uint32_t *__restrict__ slot, uint64_t capacity,
                                                         uint32_t hash_bits, const uint8_t *__restrict__ labels,
                                                         const uint64_t *__restrict__ label_off, unsigned long long *__restrict__ stats)
{
    const uint64_t j = (uint64_t)blockIdx.x * kIT + threadIdx.x;
    if (j >= cnt) return;
    const uint32_t id = (uint32_t)(first + j);
    const uint64_t l0 = label_off[id];
    uint64_t at = barcode_home(barcode_hash(labels + l0, label_off[id + 1] - l0), hash_bits, capacity);
    bool wrapped = false, placed = false;
    uint64_t k = 0;
    for (; k < capacity; ++k) {
        if (atomicCAS(slot + at, kBarcodeEmpty, id) == kBarcodeEmpty) {
            placed = true;
            break;
        }
        if (++at == capacity) {
            at = 0;
            wrapped = true;
        }
    }
    const uint64_t steps = placed ? k + 1 : capacity;
    if (steps > 1) atomicMax(stats + kStatProbe, (unsigned long long)steps);
    if (wrapped) atomicOr(stats + kStatWrapped, 1ull);
    if (!placed) atomicOr(stats + kStatError, 1ull);
}

__global__ __launch_bounds__(kIT) void k_barcode_iota(uint64_t n, uint32_t *__restrict__ dst)
{
    const uint64_t k = (uint64_t)blockIdx.x * kIT + threadIdx.x;
    if (k < n) dst[k] = (uint32_t)k;
}

// The sorted cell ids' run starts: cell_rec_off[key[p]] = p where a run starts (every cell has a survivor: every entry
// below n_cells is written), cell_rec_off[n_cells] = n.
__global__ __launch_bounds__(kIT) void k_barcode_run_starts(uint64_t n, uint64_t n_cells, const uint32_t *__restrict__ key,
                                                             uint64_t *__restrict__ cell_rec_off)
{
    const uint64_t p = (uint64_t)blockIdx.x * kIT + threadIdx.x;
    if (p > n) return;
    if (p == n) {
        cell_rec_off[n_cells] = n;
        return;
    }
    const uint32_t c = key[p];
    if (c < n_cells && (p == 0 || key[p - 1] != c)) cell_rec_off[c] = p;
}

std::mutex g_last_mu;
uint64_t g_table_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};

} // namespace

void barcode_table_last(uint64_t *out8)
{
    std::lock_guard<std::mutex> lk(g_last_mu);
    std::memcpy(out8, g_table_last, sizeof g_table_last);
}

int barcode_table_insert(uint64_t first, uint64_t cnt, uint32_t *d_slot, uint64_t capacity, uint32_t hash_bits, const uint8_t *d_labels,
                         const uint64_t *d_label_off, unsigned long long *d_stats)
{
    hipLaunchKernelGGL(k_barcode_insert, grid_of(cnt), dim3(kIT), 0, nullptr, first, cnt, d_slot, capacity, hash_bits, d_labels, d_label_off, d_stats);
    OEM_HIP(hipGetLastError());
    return OEM_OK;
}

int BarcodeIntern::init()
{
    uint64_t cap = 2;
    const uint64_t slots0 = (uint64_t)std::max<long>(knob("OEM_BARCODE_TABLE_SLOTS0", (long)kBarcodeTableSlots0), 2);
    while (cap < slots0) cap *= 2;
    hash_bits = (uint32_t)std::min<long>(std::max<long>(knob("OEM_BARCODE_HASH_BITS", 64), 0), 64);
    OEM_TRY(dev_alloc(&slot.p, cap, nullptr));
    OEM_HIP(hipMemset(slot.p, 0xff, sizeof(uint32_t) * cap));
    capacity = cap;
    OEM_TRY(dev_alloc(&stats.p, kStatWords, nullptr));
    OEM_HIP(hipMemset(stats.p, 0, sizeof(unsigned long long) * kStatWords));
    return OEM_OK;
}

void BarcodeIntern::release()
{
    slot.reset();
    labels.release();
    stats.reset();
    capacity = 0;
}

int BarcodeIntern::check_stats(const char *who)
{
    unsigned long long st[kStatWords];
    OEM_HIP(hipMemcpy(st, stats.p, sizeof st, hipMemcpyDeviceToHost));
    longest_probe = std::max<uint64_t>(longest_probe, st[kStatProbe]);
    wrapped = wrapped || st[kStatWrapped] != 0;
    if (st[kStatError])
        return fail(OEM_ERR_STATE, "%s: the barcode table is broken: a probe went round all %llu slots, or a label was not found after its insert", who,
                    (unsigned long long)capacity);
    return OEM_OK;
}

int BarcodeIntern::batch(const char *who, const uint8_t *d_bc, const uint64_t *d_bc_off, uint64_t m, uint32_t *d_cell_id)
{
    if (m == 0) return OEM_OK;
    // 1. the lookup: reads the table only
    DevBuf<uint32_t> d_miss, d_idx;
    DevBuf<uint64_t> d_at;
    OEM_TRY(dev_alloc(&d_miss.p, m + 1, nullptr));
    OEM_TRY(dev_alloc(&d_at.p, m + 1, nullptr));
    hipLaunchKernelGGL(k_barcode_lookup, grid_of(m + 1), dim3(kIT), 0, nullptr, m, (const uint32_t *)nullptr, d_bc, d_bc_off,
                       (const uint32_t *)slot.p, capacity, hash_bits, (const uint8_t *)labels.bytes.p, (const uint64_t *)labels.off.p, labels.n, 0u,
                       d_cell_id, d_miss.p, stats.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(exclusive_scan_u32(d_miss.p, d_at.p, m + 1));
    uint64_t n_miss = 0;
    OEM_HIP(hipMemcpy(&n_miss, d_at.p + m, sizeof n_miss, hipMemcpyDeviceToHost));
    OEM_TRY(check_stats(who));
    misses += n_miss;
    if (n_miss == 0) return OEM_OK;

    // 2. the misses, dense; their distinct barcodes ranked by first survivor
    OEM_TRY(dev_alloc(&d_idx.p, n_miss, nullptr));
    hipLaunchKernelGGL(k_barcode_miss_scatter, grid_of(m), dim3(kIT), 0, nullptr, m, (const uint32_t *)d_miss.p, (const uint64_t *)d_at.p, d_idx.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipStreamSynchronize(nullptr));
    d_miss.reset();
    d_at.reset();
    DevBuf<uint64_t> d_moff, d_lab_off;
    DevBuf<uint8_t> d_mblob, d_lab;
    uint64_t mbytes = 0, lab_bytes = 0;
    OEM_TRY(gather_input_names(d_idx.p, n_miss, d_bc, d_bc_off, &d_moff, &d_mblob, &mbytes));
    BarcodeCells cells;
    DevBuf<uint32_t> d_heads; // the new labels' first records among the misses, ascending
    OEM_TRY(collate_barcodes_device(who, d_mblob.p, d_moff.p, mbytes, n_miss, &cells, &d_heads));
    const uint64_t n_new = cells.n_cells;
    cells.order.reset();
    cells.cell_rec_off.reset();
    if (n_new == 0 || n_new > n_miss) return fail(OEM_ERR_STATE, "%s: %llu misses gave %llu new barcodes", who, (unsigned long long)n_miss, (unsigned long long)n_new);
    OEM_TRY(gather_input_names(d_heads.p, n_new, d_mblob.p, d_moff.p, &d_lab_off, &d_lab, &lab_bytes));
    const uint64_t first_new = labels.n;
    OEM_TRY(labels.reserve(labels.n + n_new, labels.n_bytes + lab_bytes, 1024, 4096, 0, nullptr));
    OEM_TRY(labels.append(d_lab.p, d_lab_off.p, n_new, lab_bytes));
    OEM_HIP(hipStreamSynchronize(nullptr));
    const uint64_t n_labels = labels.n;

    // 3. the load stays at or below 1/2: a table of twice the capacity (or more) from the label blob
    uint64_t from = first_new;
    if (2 * n_labels > capacity) {
        uint64_t cap = capacity, doublings = 0;
        while (2 * n_labels > cap) {
            cap *= 2;
            ++doublings;
        }
        DevBuf<uint32_t> s2;
        OEM_TRY(dev_alloc(&s2.p, cap, nullptr));
        OEM_HIP(hipMemset(s2.p, 0xff, sizeof(uint32_t) * cap));
        std::swap(slot.p, s2.p);
        capacity = cap;
        from = 0;
        ++rebuilds;
        max_doublings = std::max(max_doublings, doublings);
    }
    // 4. the insert
    OEM_TRY(barcode_table_insert(from, n_labels - from, slot.p, capacity, hash_bits, labels.bytes.p, labels.off.p, stats.p));
    // 5. the misses again
    hipLaunchKernelGGL(k_barcode_lookup, grid_of(n_miss + 1), dim3(kIT), 0, nullptr, n_miss, (const uint32_t *)d_idx.p, d_bc, d_bc_off,
                       (const uint32_t *)slot.p, capacity, hash_bits, (const uint8_t *)labels.bytes.p, (const uint64_t *)labels.off.p, n_labels, 1u,
                       d_cell_id, (uint32_t *)nullptr, stats.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipStreamSynchronize(nullptr));
    return check_stats(who);
}

int BarcodeIntern::cells(const uint32_t *d_cell_id, uint64_t n, BarcodeCells *out)
{
    DevBuf<uint32_t> d_iota, d_key_s, d_order;
    DevBuf<uint64_t> d_cro;
    DevBuf<uint8_t> tmp;
    OEM_TRY(dev_alloc(&d_iota.p, n, nullptr));
    OEM_TRY(dev_alloc(&d_key_s.p, n, nullptr));
    OEM_TRY(dev_alloc(&d_order.p, n, nullptr));
    OEM_TRY(dev_alloc(&d_cro.p, labels.n + 1, nullptr));
    hipLaunchKernelGGL(k_barcode_iota, grid_of(n), dim3(kIT), 0, nullptr, n, d_iota.p);
    OEM_HIP(hipGetLastError());
    const int bits = std::max(bits_of(labels.n - 1), 1); // a stable sort over only the bits n_cells needs
    size_t tb = 0;
    OEM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, d_cell_id, d_key_s.p, (const uint32_t *)d_iota.p, d_order.p, (int)n, 0, bits, nullptr));
    OEM_TRY(dev_alloc(&tmp.p, tb, nullptr));
    OEM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, d_cell_id, d_key_s.p, (const uint32_t *)d_iota.p, d_order.p, (int)n, 0, bits, nullptr));
    hipLaunchKernelGGL(k_barcode_run_starts, grid_of(n + 1), dim3(kIT), 0, nullptr, n, labels.n, (const uint32_t *)d_key_s.p, d_cro.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipStreamSynchronize(nullptr));
    std::swap(out->order.p, d_order.p);
    std::swap(out->cell_rec_off.p, d_cro.p);
    out->n_cells = labels.n;
    return OEM_OK;
}

int BarcodeIntern::labels_down(std::vector<uint8_t> *out_labels, std::vector<uint64_t> *out_label_off)
{
    out_labels->assign(labels.n_bytes, 0);
    out_label_off->assign(labels.n + 1, 0);
    if (labels.n_bytes) OEM_HIP(hipMemcpy(out_labels->data(), labels.bytes.p, labels.n_bytes, hipMemcpyDeviceToHost));
    if (labels.n) OEM_HIP(hipMemcpy(out_label_off->data(), labels.off.p, sizeof(uint64_t) * (labels.n + 1), hipMemcpyDeviceToHost));
    return OEM_OK;
}

void BarcodeIntern::publish_last() const
{
    std::lock_guard<std::mutex> lk(g_last_mu);
    const uint64_t v[8] = {rebuilds, longest_probe, wrapped ? 1ull : 0ull, max_doublings, capacity, labels.n, misses, 0};
    std::memcpy(g_table_last, v, sizeof v);
}

} // namespace oem
