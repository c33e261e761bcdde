// oem_barcode_table.h -- the table of barcodes seen so far, as pure host / device code: what the any-order barcoded cells
// session (oem_cells_barcodes_sort_stream.hip) interns its batches' barcodes against, and what the host walk of its rule
// (ParseCellsAnyOrderStream, oem_collate.h) uses in its place.
//
//   - open addressing with linear probing; the capacity is a power of two and at least twice the number of labels;
//   - a slot is a label's id (a uint32_t: the cell's number) or kBarcodeEmpty;
//   - the labels live in one blob in id order (label_off: n_labels + 1 offsets from 0), on the device zero-padded by 16
//     like the arena's names, so that a label can be read 8 bytes at a time;
//   - the hash is a 64-bit mix over the barcode's zero-padded 8-byte words and its length; hash_bits < 64 masks it before
//     the home slot is taken (the testing library's OEM_BARCODE_HASH_BITS): only the low hash_bits bits stay the hash's,
//     the bits above them are set, so the home slots are the table's last 2^hash_bits ones (0: the very last slot for
//     every label) and every probe of more than a step or two runs past the table's end;
//   - a probe loop ends after `capacity` steps with kBarcodeProbeError: the load never passes 1/2, so this is a broken
//     table, never an input.
// Results never depend on the hash: a label's id is given by the order of first appearance, the table only finds it.
#pragma once

#include <stdint.h>
#include <string.h>

#ifndef OEM_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define OEM_HD __host__ __device__
#else
#define OEM_HD
#endif
#endif

#include <vector>

namespace oem {

constexpr uint32_t kBarcodeEmpty = 0xffffffffu;      // a free slot; from a lookup: a miss
constexpr uint32_t kBarcodeProbeError = 0xfffffffeu; // a probe went round the whole table
constexpr uint64_t kBarcodeTableSlots0 = 1ull << 13; // the first capacity (the testing library: OEM_BARCODE_TABLE_SLOTS0)

// word w of the barcode p[0 .. len): its bytes [8 w, 8 w + 8), byte 0 in the low bits, zero past the end (8 w < len).
// On the device the blob is padded, so the word is one 8-byte load; on the host no byte past the barcode is touched.
OEM_HD inline uint64_t barcode_word(const uint8_t *p, uint64_t len, uint64_t w)
{
    const uint64_t at = 8 * w, left = len - at;
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t v;
    __builtin_memcpy(&v, p + at, 8);
    if (left < 8) v &= (1ull << (8 * left)) - 1;
    return v;
#else
    uint64_t v = 0;
    for (uint64_t b = 0; b < 8 && b < left; ++b) v |= (uint64_t)p[at + b] << (8 * b);
    return v;
#endif
}

OEM_HD inline uint64_t barcode_mix(uint64_t h)
{
    h ^= h >> 30;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27;
    h *= 0x94d049bb133111ebull;
    h ^= h >> 31;
    return h;
}

OEM_HD inline uint64_t barcode_hash(const uint8_t *p, uint64_t len)
{
    uint64_t h = 0x9e3779b97f4a7c15ull ^ len;
    for (uint64_t w = 0; 8 * w < len; ++w) h = barcode_mix(h ^ barcode_word(p, len, w));
    return barcode_mix(h);
}

// the home slot of a hash in a table of `capacity` slots
OEM_HD inline uint64_t barcode_home(uint64_t hash, uint32_t hash_bits, uint64_t capacity)
{
    if (hash_bits < 64) hash |= ~0ull << hash_bits;
    return hash & (capacity - 1);
}

// the lengths first, then the bytes 8 at a time
OEM_HD inline bool barcode_equal(const uint8_t *a, uint64_t la, const uint8_t *b, uint64_t lb)
{
    if (la != lb) return false;
    for (uint64_t w = 0; 8 * w < la; ++w)
        if (barcode_word(a, la, w) != barcode_word(b, lb, w)) return false;
    return true;
}

// The lookup: reads the table only.  The id of the barcode p[0 .. len), kBarcodeEmpty when it is not in the table,
// kBarcodeProbeError after `capacity` steps.  *steps: the slots looked at; *wrapped: the probe went past the table's end.
OEM_HD inline uint32_t barcode_table_find(const uint32_t *slot, uint64_t capacity, uint32_t hash_bits, const uint8_t *labels,
                                          const uint64_t *label_off, const uint8_t *p, uint64_t len, uint64_t *steps, bool *wrapped)
{
    uint64_t at = barcode_home(barcode_hash(p, len), hash_bits, capacity);
    for (uint64_t k = 0; k < capacity; ++k) {
        const uint32_t id = slot[at];
        if (id == kBarcodeEmpty) {
            *steps = k + 1;
            return kBarcodeEmpty;
        }
        const uint64_t l0 = label_off[id];
        if (barcode_equal(p, len, labels + l0, label_off[id + 1] - l0)) {
            *steps = k + 1;
            return id;
        }
        if (++at == capacity) {
            at = 0;
            *wrapped = true;
        }
    }
    *steps = capacity;
    return kBarcodeProbeError;
}

// The host form of the table, with its labels.  What the device does with kernels -- lookup, rebuild at twice the
// capacity when the load would pass 1/2, insert -- on plain vectors.
struct BarcodeTableHost {
    std::vector<uint32_t> slot;
    std::vector<uint8_t> labels;
    std::vector<uint64_t> label_off{0};
    uint32_t hash_bits = 64;
    uint64_t rebuilds = 0, longest_probe = 0;
    bool wrapped = false, broken = false;

    explicit BarcodeTableHost(uint64_t slots0 = kBarcodeTableSlots0, uint32_t bits = 64) : hash_bits(bits)
    {
        uint64_t cap = 2;
        while (cap < slots0) cap *= 2;
        slot.assign(cap, kBarcodeEmpty);
    }
    uint64_t n_labels() const { return label_off.size() - 1; }
    uint32_t find(const uint8_t *p, uint64_t len)
    {
        uint64_t steps = 0;
        const uint32_t id = barcode_table_find(slot.data(), slot.size(), hash_bits, labels.data(), label_off.data(), p, len, &steps, &wrapped);
        if (steps > longest_probe) longest_probe = steps;
        if (id == kBarcodeProbeError) broken = true;
        return id;
    }
    // label `id` (in the blob already, and in no slot) into the first free slot of its probe path
    void insert(uint32_t id)
    {
        const uint64_t l0 = label_off[id], cap = slot.size();
        uint64_t at = barcode_home(barcode_hash(labels.data() + l0, label_off[id + 1] - l0), hash_bits, cap);
        for (uint64_t k = 0; k < cap; ++k) {
            if (slot[at] == kBarcodeEmpty) {
                slot[at] = id;
                if (k + 1 > longest_probe) longest_probe = k + 1;
                return;
            }
            if (++at == cap) {
                at = 0;
                wrapped = true;
            }
        }
        broken = true;
    }
    // The labels [first_new, n_labels) have been appended to the blob: the table doubles until it holds all labels at a
    // load of at most 1/2 (every label is inserted again after each doubling), or only the new ones go in.
    void add_from(uint64_t first_new)
    {
        uint64_t cap = slot.size(), from = first_new;
        while (2 * n_labels() > cap) cap *= 2;
        if (cap != slot.size()) { // one rebuild, however many doublings it covers
            slot.assign(cap, kBarcodeEmpty);
            ++rebuilds;
            from = 0;
        }
        for (uint64_t id = from; id < n_labels(); ++id) insert((uint32_t)id);
    }
};

} // namespace oem
