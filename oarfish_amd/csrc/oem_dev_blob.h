// oem_dev_blob.h -- what the sessions that parse named records on the device keep there until it can be cut, once: a
// growable blob of variable-length items (DevBlob) and the arena of a session's surviving records around it
// (SurvivorArena).  The sorting names session (oem_records_stream.hip), the barcoded cells sessions
// (oem_cells_barcodes_stream.hip) and the any-order session's label table (oem_cells_barcodes_sort_stream.hip) hold
// instances of these and nothing of their own.  Everything runs on the null stream.
//
// THE PADDING INVARIANT.  A blob's bytes are allocated 16 past their capacity, off[0] == 0, and after every reserve,
// append and move_tail the 16 bytes behind n_bytes are zero; the arena's flags are allocated 8 past its capacity and
// the 8 bytes behind its n flags are zero.  That is all any reader needs.  Every reader of these blobs takes an item
// through aligned or unaligned 8- or 16-byte loads that may reach up to 15 bytes past the item's last byte, and masks
// or bounds what it loaded by the item's length: bytes_equal (k_barcode_heads), barcode_word (k_barcode_lookup,
// k_barcode_insert), load_bytes (gather_names), load_key and k_collate_validate (collate_resident, and through it
// parse_check_repeat and dedup_mark).  None of them reads a value from the padding, so it only has to be there; it is
// kept zero so that no load ever returns bytes nobody wrote.  k_flags_gather reads the flags through aligned 4-byte
// words, at most 3 bytes past the last flag.  k_stream_concat never reads an arena: bytes are appended by a
// device-to-device copy.
#pragma once

#include <algorithm>
#include <cstdint>

namespace oem {

// ---- the growth rule and the allocation sizes: host arithmetic, tested without a device (tests/native/dev_blob_main.cpp)

constexpr uint64_t kBlobPad = 16; // bytes allocated, and kept zero, behind a blob's bytes
constexpr uint64_t kFlagPad = 8;  // ... behind an arena's flags

// the capacity that follows `cap` when `need` no longer fits: geometric, and never below the instance's floor
inline uint64_t next_cap(uint64_t cap, uint64_t need, uint64_t first) { return std::max(std::max(2 * cap, need), first); }
// what is allocated for a capacity: a blob's bytes, its offsets (cap + 1 of them), an arena's flags
inline uint64_t blob_alloc_bytes(uint64_t cap_bytes) { return cap_bytes + kBlobPad; }
inline uint64_t blob_alloc_offsets(uint64_t cap) { return cap + 1; }
inline uint64_t flags_alloc_bytes(uint64_t cap) { return cap + kFlagPad; }

} // namespace oem

#ifdef __HIPCC__

#include "oem_collate_device.h"

namespace oem {

// n items of n_bytes bytes: off holds n + 1 offsets from 0, room for cap items and cap_bytes bytes.  The two capacities
// grow independently, in place; the used part is copied on the device.
struct DevBlob {
    DevBuf<uint64_t> off;
    DevBuf<uint8_t> bytes;
    uint64_t n = 0, n_bytes = 0, cap = 0, cap_bytes = 0;

    uint64_t held() const { return (off.p ? sizeof(uint64_t) * blob_alloc_offsets(cap) : 0) + (bytes.p ? blob_alloc_bytes(cap_bytes) : 0); }
    // One capacity to `to`; the previous allocation is left in *old, for a caller that grows several arrays together.
    int grow_entries(uint64_t to, DevBuf<uint64_t> *old);
    int grow_bytes(uint64_t to, DevBuf<uint8_t> *old);
    // Room for n_need items of bytes_need bytes, by next_cap over the floors first_n / first_bytes (the testing library:
    // OEM_ARENA_RECORDS0 and OEM_ARENA_BYTES0 replace every instance's).  *peak (or NULL) = max(*peak, others + the
    // bytes the blob holds while a growing part is alive twice), `others` being what its owner holds beside it.
    int reserve(uint64_t n_need, uint64_t bytes_need, uint64_t first_n, uint64_t first_bytes, uint64_t others, uint64_t *peak);
    // m items behind the n: a dense blob with m + 1 offsets from 0.  The room is the caller's to reserve.
    int append(const uint8_t *d_dense, const uint64_t *d_dense_off, uint64_t m, uint64_t dense_bytes) { return put(d_dense, d_dense_off, m, dense_bytes, n_bytes); }
    // Into an empty blob with room for them: src's items from first_entry on, whose bytes start at first_byte.
    int move_tail(const DevBlob &src, uint64_t first_entry, uint64_t first_byte);
    void release() { off.reset(); bytes.reset(); n = n_bytes = cap = cap_bytes = 0; }

private:
    int put(const uint8_t *d_bytes, const uint64_t *d_off, uint64_t m, uint64_t nb, uint64_t add);
};

// A session's survivors on the device, in the order they were appended: their records, 64-bit session-global indices,
// flags (0 or 1), names and -- as the session needs them -- cell ids and UMIs.  All arrays share `cap`; a blob's bytes
// have their own capacity.  An arena grows per part and in place, so nothing else may hold it while it is appended to.
// peak: the most device bytes it held (held(), plus a growing part alive twice).
struct SurvivorArena {
    DevBuf<oem_aln_record> rec;
    DevBuf<uint64_t> gidx;
    DevBuf<uint8_t> sec;
    DevBuf<uint32_t> cell_id;
    DevBlob names, umis;
    uint64_t n = 0, cap = 0, peak = 0;
    uint64_t first_n = 0, first_bytes = 0;
    bool with_ids = false, with_umis = false;

    SurvivorArena(uint64_t first_records, uint64_t first_blob_bytes, bool ids, bool umis_too)
        : first_n(first_records), first_bytes(first_blob_bytes), with_ids(ids), with_umis(umis_too)
    {
    }
    uint64_t own_bytes(uint64_t c) const // rec, gidx, sec and cell_id at capacity c
    {
        return c * (sizeof(oem_aln_record) + sizeof(uint64_t) + (with_ids ? sizeof(uint32_t) : 0)) + flags_alloc_bytes(c);
    }
    uint64_t held() const { return (rec.p ? own_bytes(cap) : 0) + names.held() + umis.held(); }
    int reserve(uint64_t n_need, uint64_t name_bytes_need, uint64_t umi_bytes_need);
    // a fresh arena at exactly these capacities, whatever the floors
    int make(uint64_t records, uint64_t name_bytes, uint64_t umi_bytes);
    // The batch's m survivors d_in[d_order[k]] (d_in: n_in records, the first one the session's record rec_base) with
    // their dense names, flags (or NULL: none), cell ids and UMIs, as the arena has them.  Reserves, and leaves the
    // null stream idle.
    int append(uint64_t m, const uint32_t *d_order, const oem_aln_record *d_in, uint64_t n_in, uint64_t rec_base, const uint8_t *d_names,
               const uint64_t *d_name_off, uint64_t name_bytes, const uint8_t *d_sec, const uint32_t *d_cell_id, const uint8_t *d_umis,
               const uint64_t *d_umi_off, uint64_t umi_bytes);
    // Into an empty arena (a collated session's: no cell ids) with room for them: old's survivors from t on, whose names
    // and UMIs start at these bytes (old's offsets at t).
    int take_tail(const SurvivorArena &old, uint64_t t, uint64_t first_name_byte, uint64_t first_umi_byte);
    void release() { rec.reset(); gidx.reset(); sec.reset(); cell_id.reset(); names.release(); umis.release(); n = cap = 0; }

private:
    int grow_entries(uint64_t to);
};

} // namespace oem

#endif // __HIPCC__
