// oem_collate_device.hip -- oem_collate_names: a cell's alignment records collated by read name on the device.
//
// The rule is oem_collate.h's (alignment_parser.rs:170-241 and :301-437).  The cells are taken in batches of at most
// kCollateBatchRecords records (whole cells; a larger cell is a batch of its own), which bounds the device memory of a
// call.  A batch's names go up through the pinned upload lanes of oem_filter_device.h in chunks cut at cell boundaries;
// behind each chunk, on its lane, run k_collate_validate (an empty name, a 0 byte) and the first key kernel, so both
// overlap the next chunk's copy.  Nothing after the upload knows of the chunks.
//
// A batch is collate_resident (oem_collate_device.h): it leaves order, the batch's group_off and cell_group_off on the
// device.  oem_collate_names copies them to the caller's arrays; oem_em_run_cells_records_names_sparse
// (oem_cells_records.hip) gathers and filters the batch's records behind them and copies only what its caller asked for.
//
// kCollateSort is a most-significant-key-first radix sort over 8-byte keys (collate_key), on the records that are still
// undecided:
//   - the start is, per cell, the primaries in index order and then the secondaries in index order (k_collate_start,
//     from one scan of the secondary flags).  Every later step is a stable sort, so records with identical names stay in
//     that order: rules 2 and 3 of the order cost no pass of their own;
//   - a run is a maximal stretch of positions whose records agreed in every key so far; it never crosses a cell (the
//     first runs are the cells).  Round r builds key r of every undecided record (k_collate_keys), sorts the undecided
//     records by key (hipcub::DeviceRadixSort, only over the bit range in which the round's keys differ at all -- none:
//     no sort) and then stably by run number, which puts every run back on its own positions in key order;
//   - k_collate_recut compares neighbours, writes the records to their positions in `order` and marks where a new run
//     starts (those marks, accumulated, are the group starts).  Where two neighbours of a run have the same key it
//     compares the rest of their names: a run without a differing pair holds one name and is finished -- a read's
//     primary and secondaries settle in the round that separates them from the other reads, not at their name's end.
//     One hipcub::DeviceScan numbers the runs, k_collate_mark / k_collate_keep find the runs that still hold two names,
//     a second, packed scan and k_collate_compact renumber those runs and close the ranks.
// The loop ends when nothing is undecided, at the latest in the round of the longest name's last byte.
// kCollateAdjacent replaces all of that by k_collate_adjacent (compare with the previous record, key by key).  Both end
// in one scan of the marks: group_off, and cell_group_off sampled at the cells' first records (k_collate_finish).
//
// k_collate_keys is a gather: 8 bytes at an arbitrary byte offset per record.  It reads the two aligned 8-byte words
// around them (the blob's base is aligned, the blob is padded), shifts them together and byte-swaps; there is no
// unaligned or byte-wide access.  The order of the gather is the current order of the records, so it is coalesced only
// where the input is collated already.
#include <hipcub/hipcub.hpp>

#include "oem_collate_device.h"
#include "oem_filter_device.h"

namespace oem {

namespace {

constexpr int kCT = 256;
constexpr uint64_t kCollateChunkBytes = 64ull << 20;    // name bytes per upload chunk (the test-only library: OEM_COLLATE_CHUNK_BYTES)
constexpr uint64_t kCollateBatchRecords = 1ull << 27;   // records per batch (the test-only library: OEM_COLLATE_BATCH_RECORDS)

thread_local double g_collate_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
thread_local double g_barcodes_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};

struct U32ToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};
struct U8ToU64 {
    __host__ __device__ uint64_t operator()(uint8_t v) const { return v != 0; }
};

__device__ __forceinline__ uint64_t tid64() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }

// the cell of record i: the first c with cell_off[c + 1] > i (cells may be empty)
__device__ __forceinline__ uint32_t cell_of(const unsigned long long *__restrict__ cell_off, uint32_t n_cells, uint64_t i)
{
    uint32_t lo = 0, hi = n_cells - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cell_off[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// collate_key of the name at bytes [b, e) of the blob, through aligned words (names is 8-byte aligned and padded by 16)
__device__ __forceinline__ uint64_t load_key(const uint8_t *__restrict__ names, uint64_t b, uint64_t e, uint64_t round)
{
    const uint64_t at = b + 8 * round;
    if (at >= e) return 0;
    const uint64_t *w = (const uint64_t *)(names + (at & ~7ull));
    const uint32_t sh = (uint32_t)(at & 7u) * 8u;
    uint64_t v = w[0] >> sh;
    if (sh && (at & ~7ull) + 8 < e) v |= w[1] << (64u - sh);
    const uint64_t n = e - at;
    if (n < 8) v &= (1ull << (8 * n)) - 1;
    return __builtin_bswap64(v);
}

// The start of the sort over the batch's m records (positions = record indices of the batch): run = cell, pos = the
// identity, and ord = per cell the primaries in index order, then the secondaries.  sec_scan: the exclusive scan of
// secondary != 0 (m + 1 entries), or NULL with secondary.
__global__ __launch_bounds__(kCT) void k_collate_start(uint64_t m, const unsigned long long *__restrict__ cell_off, uint32_t n_cells,
                                                        const uint8_t *__restrict__ sec, const uint64_t *__restrict__ sec_scan,
                                                        uint32_t *__restrict__ ord, uint32_t *__restrict__ pos, uint32_t *__restrict__ run)
{
    const uint64_t i = tid64();
    if (i >= m) return;
    const uint32_t c = cell_of(cell_off, n_cells, i);
    pos[i] = (uint32_t)i;
    run[i] = c;
    uint64_t at = i;
    if (sec) {
        const uint64_t c0 = cell_off[c], c1 = cell_off[c + 1];
        const uint64_t sec_before = sec_scan[i] - sec_scan[c0], sec_cell = sec_scan[c1] - sec_scan[c0];
        at = sec[i] ? c0 + ((c1 - c0) - sec_cell) + sec_before : c0 + ((i - c0) - sec_before);
    }
    ord[at] = (uint32_t)i;
}

// Records [r0, r1) of the batch and their bytes [b0, b1) of the blob, one upload chunk: the first record with an empty
// name -> bad[1], the first with a 0 byte -> bad[0] (indices of the call: rec_base + the batch's).
__global__ __launch_bounds__(kCT) void k_collate_validate(const uint8_t *__restrict__ names, uint64_t b0, uint64_t b1,
                                                           const uint64_t *__restrict__ off, uint64_t off_base, uint64_t r0, uint64_t r1,
                                                           uint64_t rec_base, unsigned long long *__restrict__ bad)
{
    const uint64_t t = tid64();
    if (r0 + t < r1 && off[r0 + t + 1] == off[r0 + t]) atomicMin(&bad[1], (unsigned long long)(rec_base + r0 + t));
    const uint64_t wd = (b0 >> 4) + t;
    if (wd * 16 >= b1) return;
    const uint4 v = *(const uint4 *)(names + wd * 16);
    const uint32_t x[4] = {v.x, v.y, v.z, v.w};
    for (int q = 0; q < 4; ++q) {
        if (!((x[q] - 0x01010101u) & ~x[q] & 0x80808080u)) continue;
        for (int k = 0; k < 4; ++k) {
            const uint64_t p = wd * 16 + q * 4 + k;
            if (p < b0 || p >= b1 || ((x[q] >> (8 * k)) & 0xffu)) continue;
            uint64_t lo = r0, hi = r1 - 1; // the record that holds byte p: the last i with off[i] <= p
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo + 1) / 2;
                if (off[mid] - off_base <= p) lo = mid;
                else hi = mid - 1;
            }
            atomicMin(&bad[0], (unsigned long long)(rec_base + lo));
        }
    }
}

// key[j] = key `round` of the record at rank j, for the ranks [j0, j1); or_and[0] |= and or_and[1] &= every key.
__global__ __launch_bounds__(kCT) void k_collate_keys(uint64_t j0, uint64_t j1, const uint32_t *__restrict__ ord,
                                                       const uint8_t *__restrict__ names, const uint64_t *__restrict__ off,
                                                       uint64_t off_base, uint64_t round, uint64_t *__restrict__ key,
                                                       unsigned long long *__restrict__ or_and)
{
    const uint64_t j = j0 + tid64();
    unsigned long long o = 0ull, a = ~0ull;
    if (j < j1) {
        const uint32_t r = ord[j];
        const uint64_t k = load_key(names, off[r] - off_base, off[r + 1] - off_base, round);
        key[j] = k;
        o = a = k;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        o |= __shfl_xor(o, d, 64);
        a &= __shfl_xor(a, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (o) atomicOr(&or_and[0], o);
        if (a != ~0ull) atomicAnd(&or_and[1], a);
    }
}

__global__ __launch_bounds__(kCT) void k_collate_iota(uint64_t n, uint32_t *__restrict__ dst)
{
    const uint64_t j = tid64();
    if (j < n) dst[j] = (uint32_t)j;
}

__global__ __launch_bounds__(kCT) void k_collate_gather(uint64_t n, const uint32_t *__restrict__ src, const uint32_t *__restrict__ perm,
                                                         uint32_t *__restrict__ dst)
{
    const uint64_t j = tid64();
    if (j < n) dst[j] = src[perm[j]];
}

// The names of records ra and rb agree in their keys 0 .. round: do they agree in every later key too?
__device__ __forceinline__ bool same_rest(const uint8_t *__restrict__ names, const uint64_t *__restrict__ off, uint64_t off_base,
                                          uint32_t ra, uint32_t rb, uint64_t round)
{
    const uint64_t a0 = off[ra] - off_base, a1 = off[ra + 1] - off_base, b0 = off[rb] - off_base, b1 = off[rb + 1] - off_base;
    if (a1 - a0 != b1 - b0) return false;
    for (uint64_t r = round + 1; 8 * r < a1 - a0; ++r)
        if (load_key(names, a0, a1, r) != load_key(names, b0, b1, r)) return false;
    return true;
}

// After the sorts, rank j of the n undecided holds the record that was at rank perm[j].  It goes to its position in
// `order`; a rank that starts a run (another cell, another run before, another key now) is marked in `head` and in
// flags[j]; a rank that continues a run with ANOTHER name than its predecessor's is marked in unres[j].  ord_out[j]: the
// record, for k_collate_compact.
__global__ __launch_bounds__(kCT) void k_collate_recut(uint64_t n, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ key,
                                                        const uint32_t *__restrict__ run, const uint32_t *__restrict__ ord,
                                                        const uint32_t *__restrict__ pos, const uint8_t *__restrict__ names,
                                                        const uint64_t *__restrict__ off, uint64_t off_base, uint64_t round,
                                                        uint32_t *__restrict__ order, uint32_t *__restrict__ head,
                                                        uint32_t *__restrict__ ord_out, uint64_t *__restrict__ flags,
                                                        uint32_t *__restrict__ unres)
{
    const uint64_t j = tid64();
    if (j >= n) return;
    const uint32_t o = perm[j], rec = ord[o], p = pos[j];
    const uint64_t k = key[o];
    bool h = true, u = false;
    if (j > 0) {
        const uint32_t o_prev = perm[j - 1];
        h = run[j] != run[j - 1] || k != key[o_prev];
        u = !h && !collate_key_is_last(k) && !same_rest(names, off, off_base, ord[o_prev], rec, round);
    }
    order[p] = rec;
    if (h) head[p] = 1u;
    ord_out[j] = rec;
    flags[j] = h ? 1ull : 0ull;
    unres[j] = u ? 1u : 0u;
}

// runs = the inclusive scan of the run starts: rank j is in this round's run runs[j] - 1.  A run that holds two names
// goes on (mixed[run] = 1); every other run holds one name and is finished.
__global__ __launch_bounds__(kCT) void k_collate_mark(uint64_t n, const uint32_t *__restrict__ unres, const uint64_t *__restrict__ runs,
                                                       uint32_t *__restrict__ mixed)
{
    const uint64_t j = tid64();
    if (j < n && unres[j]) mixed[runs[j] - 1] = 1u;
}

// flags[j]: low word 1 when rank j stays undecided (its run is mixed), high word 1 when it also starts its run
__global__ __launch_bounds__(kCT) void k_collate_keep(uint64_t n, const uint64_t *__restrict__ runs, const uint32_t *__restrict__ mixed,
                                                       uint64_t *__restrict__ flags)
{
    const uint64_t j = tid64();
    if (j >= n) return;
    const bool keep = mixed[runs[j] - 1] != 0, h = flags[j] != 0;
    flags[j] = (keep ? 1ull : 0ull) | (keep && h ? 1ull << 32 : 0ull);
}

// scan = the inclusive scan of flags: the undecided close ranks, their runs are renumbered from 0.
__global__ __launch_bounds__(kCT) void k_collate_compact(uint64_t n, const uint64_t *__restrict__ flags, const uint64_t *__restrict__ scan,
                                                          const uint32_t *__restrict__ pos, const uint32_t *__restrict__ ord_in,
                                                          uint32_t *__restrict__ pos_out, uint32_t *__restrict__ ord_out,
                                                          uint32_t *__restrict__ run_out)
{
    const uint64_t j = tid64();
    if (j >= n || !(flags[j] & 1ull)) return;
    const uint64_t s = scan[j];
    const uint32_t d = (uint32_t)(s & 0xffffffffull) - 1u;
    pos_out[d] = pos[j];
    ord_out[d] = ord_in[j];
    run_out[d] = (uint32_t)(s >> 32) - 1u;
}

// kCollateAdjacent for the records [r0, r1) of the batch: the identity order, a mark where a cell starts or the name
// differs from the previous record's.
__global__ __launch_bounds__(kCT) void k_collate_adjacent(uint64_t r0, uint64_t r1, const uint8_t *__restrict__ names,
                                                           const uint64_t *__restrict__ off, uint64_t off_base,
                                                           const unsigned long long *__restrict__ cell_off, uint32_t n_cells,
                                                           uint32_t *__restrict__ order, uint32_t *__restrict__ head)
{
    const uint64_t i = r0 + tid64();
    if (i >= r1) return;
    order[i] = (uint32_t)i;
    const uint32_t c = cell_of(cell_off, n_cells, i);
    bool h = i == cell_off[c];
    if (!h) {
        const uint64_t a0 = off[i - 1] - off_base, a1 = off[i] - off_base, b1 = off[i + 1] - off_base;
        h = a1 - a0 != b1 - a1;
        for (uint64_t r = 0; !h; ++r) {
            const uint64_t ka = load_key(names, a0, a1, r), kb = load_key(names, a1, b1, r);
            if (ka != kb) h = true;
            else if (collate_key_is_last(ka)) break;
        }
    }
    head[i] = h ? 1u : 0u;
}

// gidx: the exclusive scan of head (m + 1 entries).  The marks become group_off (positions from pos_base, closed by
// pos_base + m), the order's entries record indices from order_base, and the cells' first groups are sampled.
__global__ __launch_bounds__(kCT) void k_collate_finish(uint64_t m, uint32_t n_cells, const uint32_t *__restrict__ head,
                                                         const uint64_t *__restrict__ gidx, const unsigned long long *__restrict__ cell_off,
                                                         uint64_t order_base, uint64_t pos_base, uint64_t group_base,
                                                         uint32_t *__restrict__ order, uint64_t *__restrict__ group_off,
                                                         uint64_t *__restrict__ cell_group_off)
{
    const uint64_t i = tid64();
    if (i <= n_cells) cell_group_off[i] = group_base + gidx[cell_off[i]];
    if (i == 0) group_off[gidx[m]] = pos_base + m; // (gidx[m] = the batch's groups, at most m: the buffer has m + 1 entries)
    if (i >= m) return;
    order[i] += (uint32_t)order_base;
    if (head[i]) group_off[gidx[i]] = pos_base + i;
}

// ---- cells from barcodes (oem_collate.h's barcode rule), behind the sort of all records as one cell: `sorted` is the
// stable order by barcode bytes, run_off (n_runs + 1, closed by n) the positions where a barcode starts.

// the run of position p: the last r with run_off[r] <= p
__device__ __forceinline__ uint64_t run_of(const uint64_t *__restrict__ run_off, uint64_t n_runs, uint64_t p)
{
    uint64_t lo = 0, hi = n_runs - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (run_off[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// a run's head is its first record: its smallest, the sort being stable
__global__ __launch_bounds__(kCT) void k_barcode_heads(uint64_t n_runs, const uint32_t *__restrict__ sorted, const uint64_t *__restrict__ run_off,
                                                        uint32_t *__restrict__ head, uint32_t *__restrict__ idx)
{
    const uint64_t r = tid64();
    if (r >= n_runs) return;
    head[r] = sorted[run_off[r]];
    idx[r] = (uint32_t)r;
}

// run_of_rank: the runs sorted by head.  len[k] = the length of the run of rank k (len[n_runs] = 0, for the scan).
__global__ __launch_bounds__(kCT) void k_barcode_lengths(uint64_t n_runs, const uint32_t *__restrict__ run_of_rank,
                                                          const uint64_t *__restrict__ run_off, uint64_t *__restrict__ len,
                                                          uint32_t *__restrict__ rank_of_run)
{
    const uint64_t k = tid64();
    if (k > n_runs) return;
    if (k == n_runs) {
        len[k] = 0;
        return;
    }
    const uint32_t r = run_of_rank[k];
    len[k] = run_off[r + 1] - run_off[r];
    rank_of_run[r] = (uint32_t)k;
}

// every run to the place of its rank: cell_rec_off is the exclusive scan of len
__global__ __launch_bounds__(kCT) void k_barcode_scatter(uint64_t n, uint64_t n_runs, const uint32_t *__restrict__ sorted,
                                                          const uint64_t *__restrict__ run_off, const uint32_t *__restrict__ rank_of_run,
                                                          const uint64_t *__restrict__ cell_rec_off, uint32_t *__restrict__ order_bc)
{
    const uint64_t p = tid64();
    if (p >= n) return;
    const uint64_t r = run_of(run_off, n_runs, p);
    order_bc[cell_rec_off[rank_of_run[r]] + (p - run_off[r])] = sorted[p];
}

// ---- the gather of names that are resident

// len[k] = the length of the name of record order[k]; len[m] = 0
__global__ __launch_bounds__(kCT) void k_names_lengths(uint64_t m, const uint32_t *__restrict__ order, const uint64_t *__restrict__ off,
                                                        uint64_t *__restrict__ len)
{
    const uint64_t k = tid64();
    if (k > m) return;
    len[k] = k < m ? off[(uint64_t)order[k] + 1] - off[order[k]] : 0ull;
}

// up to 8 bytes from byte `at` of the blob through its aligned words, byte 0 in the low bits (the blob is 8-byte aligned
// and padded: the second word is read only when the bytes reach into it)
__device__ __forceinline__ uint64_t load_bytes(const uint8_t *__restrict__ blob, uint64_t at, uint32_t n)
{
    const uint64_t *w = (const uint64_t *)(blob + (at & ~7ull));
    const uint32_t sh = (uint32_t)(at & 7u) * 8u;
    uint64_t v = w[0] >> sh;
    if (sh && (at & 7u) + n > 8u) v |= w[1] << (64u - sh);
    if (n < 8) v &= (1ull << (8 * n)) - 1;
    return v;
}

// One lane per 8-byte word of the gathered blob, so the stores are coalesced and no access is byte-wide: word j holds
// the bytes [8 j, 8 j + 8) of the concatenation of the names of order[0 .. m), name k at out_off[k] - off_base.  A word
// may take its bytes from several names (a name can be one byte long); the lane walks them.  The record of the
// workgroup's first byte is searched once among all m, each lane's own among the few that a workgroup's 2 KiB can hold.
// Bytes past out_bytes are written as 0.  with_empty: names may be empty (the UMIs of a session's survivors), so no
// count of records bounds a lane's search; an empty name is passed by, as it holds no byte.
__global__ __launch_bounds__(kCT) void k_names_gather(uint64_t n_words, uint64_t out_bytes, uint64_t m, const uint32_t *__restrict__ order,
                                                       const uint8_t *__restrict__ names, const uint64_t *__restrict__ off,
                                                       const uint64_t *__restrict__ out_off, uint64_t off_base, uint32_t with_empty,
                                                       uint64_t *__restrict__ out)
{
    const uint64_t j = tid64();
    if (j >= n_words) return;
    uint64_t lo = 0, hi = m - 1; // the record that holds byte p: the last k with out_off[k] - off_base <= p
    {
        const uint64_t p0 = (uint64_t)blockIdx.x * kCT * 8;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (out_off[mid] - off_base <= p0) lo = mid;
            else hi = mid - 1;
        }
        hi = !with_empty && lo + (uint64_t)kCT * 8 < m - 1 ? lo + (uint64_t)kCT * 8 : m - 1; // (names that are never empty: a byte each at least)
    }
    uint64_t p = 8 * j;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (out_off[mid] - off_base <= p) lo = mid;
        else hi = mid - 1;
    }
    uint64_t k = lo, v = 0;
    const uint64_t end = 8 * j + 8 < out_bytes ? 8 * j + 8 : out_bytes;
    while (p < end) {
        const uint64_t k0 = out_off[k] - off_base, k1 = out_off[k + 1] - off_base;
        const uint32_t n = (uint32_t)((k1 < end ? k1 : end) - p);
        v |= load_bytes(names, off[order[k]] + (p - k0), n) << (8 * (p - 8 * j));
        p += n;
        ++k;
    }
    out[j] = v;
}

// The flags likewise, eight records per lane: out word j = the flags of order[8 j .. 8 j + 8), 0 past m.  The source is
// read through its aligned 4-byte words.
__global__ __launch_bounds__(kCT) void k_flags_gather(uint64_t n_words, uint64_t m, const uint32_t *__restrict__ order,
                                                       const uint8_t *__restrict__ sec, uint64_t *__restrict__ out)
{
    const uint64_t j = tid64();
    if (j >= n_words) return;
    uint64_t v = 0;
    for (uint32_t b = 0; b < 8; ++b) {
        const uint64_t k = 8 * j + b;
        if (k >= m) break;
        const uint32_t r = order[k];
        const uint32_t w = ((const uint32_t *)sec)[r >> 2];
        v |= (uint64_t)(((w >> (8 * (r & 3u))) & 0xffu) != 0) << (8 * b);
    }
    out[j] = v;
}

inline dim3 grid_for(uint64_t n) { return dim3((unsigned)std::max<uint64_t>((n + kCT - 1) / kCT, 1)); }

// a device buffer that only grows (the scans' and sorts' temporary storage)
struct Scratch {
    void *p = nullptr;
    size_t cap = 0;
    hipStream_t st = nullptr;
    ~Scratch() { (void)hipFree(p); }
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return OEM_OK;
        if (p) OEM_HIP(hipStreamSynchronize(st));
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
        OEM_HIP(hipMalloc(&p, bytes));
        cap = bytes;
        return OEM_OK;
    }
};

template <typename K>
int sort_pairs(Scratch &sc, const K *key_in, K *key_out, const uint32_t *val_in, uint32_t *val_out, uint64_t n, int bit0, int bit1,
               hipStream_t st)
{
    size_t tb = 0;
    OEM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, key_in, key_out, val_in, val_out, (int)n, bit0, bit1, st));
    OEM_TRY(sc.ensure(tb ? tb : 1));
    tb = sc.cap;
    OEM_HIP(hipcub::DeviceRadixSort::SortPairs(sc.p, tb, key_in, key_out, val_in, val_out, (int)n, bit0, bit1, st));
    return OEM_OK;
}

template <typename In>
int scan_u64(Scratch &sc, bool inclusive, In in, uint64_t *out, uint64_t n, hipStream_t st)
{
    size_t tb = 0;
    if (inclusive) OEM_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, tb, in, out, (int)n, st));
    else OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n, st));
    OEM_TRY(sc.ensure(tb ? tb : 1));
    tb = sc.cap;
    if (inclusive) OEM_HIP(hipcub::DeviceScan::InclusiveSum(sc.p, tb, in, out, (int)n, st));
    else OEM_HIP(hipcub::DeviceScan::ExclusiveSum(sc.p, tb, in, out, (int)n, st));
    return OEM_OK;
}

inline int bits_of(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

} // namespace

int collate_resident(const CollateInput &cc, uint32_t c0, uint32_t c1, uint64_t order_base, uint64_t pos_base, uint64_t group_base,
                     double *info, CollateResident *out)
{
    const uint32_t nc = c1 - c0;
    const uint64_t rec_base = cc.cell_rec_off[c0], m = cc.cell_rec_off[c1] - rec_base;
    const bool resident = cc.d_names != nullptr; // the device form: the names are here and checked already
    const uint64_t off_base = resident ? cc.d_off_base : cc.name_off[rec_base];
    const uint64_t n_bytes = resident ? cc.d_n_bytes : cc.name_off[rec_base + m] - off_base;
    const bool has_sec = resident ? cc.d_secondary != nullptr : cc.secondary != nullptr;
    const bool sorting = cc.mode == kCollateSort;

    // the upload chunks: whole cells, at most chunk_bytes of names unless one cell has more
    std::vector<uint64_t> byte_cut{0}, rec_cut{0};
    std::vector<unsigned long long> cell_off(nc + 1);
    if (cc.cut_records && !resident) { // one cell of everything: cut wherever a record ends
        const uint64_t *off = cc.name_off + rec_base;
        cell_off[0] = 0;
        for (uint64_t r = 0; r < m;) {
            uint64_t r1 = (uint64_t)(std::upper_bound(off + r + 1, off + m + 1, off[r] + cc.chunk_bytes) - off) - 1;
            r1 = std::max(r1, r + 1);
            if (r1 < m) {
                byte_cut.push_back(off[r1] - off_base);
                rec_cut.push_back(r1);
            }
            r = r1;
        }
        cell_off[nc] = m;
        byte_cut.push_back(n_bytes);
        rec_cut.push_back(m);
    } else {
        uint64_t start_b = 0, start_r = 0;
        for (uint32_t c = c0; c < c1; ++c) {
            const uint64_t r0 = cc.cell_rec_off[c] - rec_base, r1 = cc.cell_rec_off[c + 1] - rec_base;
            cell_off[c - c0] = r0;
            if (resident) continue;
            const uint64_t b0 = cc.name_off[rec_base + r0] - off_base, b1 = cc.name_off[rec_base + r1] - off_base;
            if (r0 > start_r && b1 - start_b > cc.chunk_bytes) {
                byte_cut.push_back(b0);
                rec_cut.push_back(r0);
                start_b = b0;
                start_r = r0;
            }
        }
        cell_off[nc] = m;
        byte_cut.push_back(n_bytes);
        rec_cut.push_back(m);
    }
    const uint64_t n_chunks = byte_cut.size() - 1;

    Stream main;
    OEM_HIP(hipStreamCreateWithFlags(&main.s, hipStreamNonBlocking));
    hipStream_t st = main.s;
    Scratch sc;
    sc.st = st;
    DevBuf<uint8_t> d_names_own, d_sec_own;
    DevBuf<uint64_t> d_off_own, d_key, d_key_s, d_flags, d_scan, d_cgo; // (d_key_s and d_cgo are handed to `out` in the end)
    DevBuf<unsigned long long> d_cell_off, d_words; // d_words: [0] zero byte, [1] empty name, [2] or, [3] and
    DevBuf<uint32_t> d_order, d_head, d_iota, d_perm1, d_perm2, d_run1, d_run1_s, d_pos[2], d_ord[2], d_run[2];
    if (!resident) {
        OEM_TRY(dev_alloc(&d_names_own.p, n_bytes + 16, nullptr));
        OEM_TRY(dev_alloc(&d_off_own.p, m + 1, nullptr));
    }
    OEM_TRY(dev_alloc(&d_cell_off.p, nc + 1, nullptr));
    OEM_TRY(dev_alloc(&d_words.p, 4, nullptr));
    OEM_TRY(dev_alloc(&d_order.p, m, nullptr));
    OEM_TRY(dev_alloc(&d_head.p, m + 1, nullptr));
    OEM_TRY(dev_alloc(&d_scan.p, m + 1, nullptr));
    OEM_TRY(dev_alloc(&d_key_s.p, m + 1, nullptr)); // (group_off of the batch in the end)
    OEM_TRY(dev_alloc(&d_cgo.p, nc + 1, nullptr));
    if (sorting) {
        OEM_TRY(dev_alloc(&d_key.p, m, nullptr));
        OEM_TRY(dev_alloc(&d_flags.p, m, nullptr));
        OEM_TRY(dev_alloc(&d_iota.p, m, nullptr));
        OEM_TRY(dev_alloc(&d_perm1.p, m, nullptr));
        OEM_TRY(dev_alloc(&d_perm2.p, m, nullptr));
        OEM_TRY(dev_alloc(&d_run1.p, m, nullptr));
        OEM_TRY(dev_alloc(&d_run1_s.p, m, nullptr));
        for (int k = 0; k < 2; ++k) {
            OEM_TRY(dev_alloc(&d_pos[k].p, m, nullptr));
            OEM_TRY(dev_alloc(&d_ord[k].p, m, nullptr));
            OEM_TRY(dev_alloc(&d_run[k].p, m, nullptr));
        }
        if (has_sec && !resident) OEM_TRY(dev_alloc(&d_sec_own.p, m + 1, nullptr));
    }
    struct { const uint8_t *p; } d_names{resident ? cc.d_names : d_names_own.p}, d_sec{resident ? cc.d_secondary : d_sec_own.p};
    struct { const uint64_t *p; } d_off{resident ? cc.d_name_off : d_off_own.p};
    Event ev[3];
    if (cc.timing)
        for (auto &e : ev) OEM_HIP(hipEventCreate(&e.e));

    // what the chunks' kernels need before the first name arrives
    const unsigned long long words0[4] = {kNoRecord, kNoRecord, 0ull, ~0ull};
    OEM_HIP(hipMemcpyAsync(d_words.p, words0, sizeof words0, hipMemcpyHostToDevice, st));
    if (!resident) OEM_HIP(hipMemcpyAsync(d_off_own.p, cc.name_off + rec_base, sizeof(uint64_t) * (m + 1), hipMemcpyHostToDevice, st));
    OEM_HIP(hipMemcpyAsync(d_cell_off.p, cell_off.data(), sizeof(unsigned long long) * (nc + 1), hipMemcpyHostToDevice, st));
    OEM_HIP(hipMemsetAsync(d_head.p, 0, sizeof(uint32_t) * (m + 1), st));
    if (!resident) OEM_HIP(hipMemsetAsync(d_names_own.p + n_bytes, 0, 16, st));
    if (sorting) {
        if (has_sec) {
            if (!resident) {
                OEM_HIP(hipMemcpyAsync(d_sec_own.p, cc.secondary + rec_base, m, hipMemcpyHostToDevice, st));
                OEM_HIP(hipMemsetAsync(d_sec_own.p + m, 0, 1, st));
            }
            hipcub::TransformInputIterator<uint64_t, U8ToU64, const uint8_t *> in(d_sec.p, U8ToU64());
            OEM_TRY(scan_u64(sc, false, in, d_scan.p, m + 1, st));
        }
        hipLaunchKernelGGL(k_collate_start, grid_for(m), dim3(kCT), 0, st, m, (const unsigned long long *)d_cell_off.p, nc,
                           (const uint8_t *)d_sec.p, (const uint64_t *)(has_sec ? d_scan.p : nullptr), d_ord[0].p, d_pos[0].p,
                           d_run[0].p);
        OEM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_collate_iota, grid_for(m), dim3(kCT), 0, st, m, d_iota.p);
        OEM_HIP(hipGetLastError());
    }
    OEM_HIP(hipStreamSynchronize(st));

    // the names, chunk by chunk; behind each chunk its checks and its share of round 0 (or of the adjacent cut)
    float ms[6] = {0, 0, 0, 0, 0, 0};
    if (resident) { // no lanes: round 0's keys (or the adjacent cut) over the whole batch
        if (sorting)
            hipLaunchKernelGGL(k_collate_keys, grid_for(m), dim3(kCT), 0, st, (uint64_t)0, m, (const uint32_t *)d_ord[0].p,
                               (const uint8_t *)d_names.p, (const uint64_t *)d_off.p, off_base, (uint64_t)0, d_key.p, d_words.p + 2);
        else
            hipLaunchKernelGGL(k_collate_adjacent, grid_for(m), dim3(kCT), 0, st, (uint64_t)0, m, (const uint8_t *)d_names.p,
                               (const uint64_t *)d_off.p, off_base, (const unsigned long long *)d_cell_off.p, nc, d_order.p, d_head.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipStreamSynchronize(st));
    } else
    OEM_TRY(filter_upload_measure<uint8_t>(
        cc.names + off_base, d_names_own.p, byte_cut.data(), n_chunks, 1, cc.timing ? ms : nullptr,
        [&](hipStream_t lane, uint64_t g0, uint64_t) {
            const uint64_t b0 = byte_cut[g0], b1 = byte_cut[g0 + 1], r0 = rec_cut[g0], r1 = rec_cut[g0 + 1];
            const uint64_t words = b1 > b0 ? ((b1 + 15) >> 4) - (b0 >> 4) : 0;
            hipLaunchKernelGGL(k_collate_validate, grid_for(std::max(words, r1 - r0)), dim3(kCT), 0, lane, (const uint8_t *)d_names.p, b0,
                               b1, (const uint64_t *)d_off.p, off_base, r0, r1, rec_base, d_words.p);
            if (sorting)
                hipLaunchKernelGGL(k_collate_keys, grid_for(r1 - r0), dim3(kCT), 0, lane, r0, r1, (const uint32_t *)d_ord[0].p,
                                   (const uint8_t *)d_names.p, (const uint64_t *)d_off.p, off_base, (uint64_t)0, d_key.p, d_words.p + 2);
            else
                hipLaunchKernelGGL(k_collate_adjacent, grid_for(r1 - r0), dim3(kCT), 0, lane, r0, r1, (const uint8_t *)d_names.p,
                                   (const uint64_t *)d_off.p, off_base, (const unsigned long long *)d_cell_off.p, nc, d_order.p, d_head.p);
        }));
    info[1] += resident ? 0.0 : (double)n_chunks;
    info[3] += ms[0];
    info[4] += ms[1];
    info[6] += ms[5];

    unsigned long long words[4];
    OEM_HIP(hipMemcpy(words, d_words.p, sizeof words, hipMemcpyDeviceToHost));
    if (words[0] != kNoRecord || words[1] != kNoRecord) {
        if (words[1] < words[0]) return fail(OEM_ERR_ARG, "%s: record %llu has an empty %s", cc.who, words[1], cc.what);
        return fail(OEM_ERR_ARG, "%s: the %s of record %llu contains a 0 byte", cc.who, cc.what, words[0]);
    }

    if (cc.timing) OEM_HIP(hipEventRecord(ev[0].e, st));
    if (sorting) {
        uint64_t n = m, run_max = nc - 1, round = 0, sorted_rounds = 0;
        int a = 0; // the side of pos / run that is current (ord: always side 0 at a round's start)
        for (;; ++round) {
            if (round > 0) {
                OEM_HIP(hipMemsetAsync(d_words.p + 2, 0, sizeof(unsigned long long), st));
                OEM_HIP(hipMemsetAsync(d_words.p + 3, 0xff, sizeof(unsigned long long), st));
                hipLaunchKernelGGL(k_collate_keys, grid_for(n), dim3(kCT), 0, st, (uint64_t)0, n, (const uint32_t *)d_ord[0].p,
                                   (const uint8_t *)d_names.p, (const uint64_t *)d_off.p, off_base, round, d_key.p, d_words.p + 2);
                OEM_HIP(hipGetLastError());
                OEM_HIP(hipMemcpyAsync(words + 2, d_words.p + 2, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
                OEM_HIP(hipStreamSynchronize(st));
            }
            const uint64_t differ = words[2] & ~words[3]; // the bits in which two of the round's keys differ
            const uint32_t *perm = d_iota.p;
            if (differ) {
                ++sorted_rounds;
                OEM_TRY(sort_pairs<uint64_t>(sc, d_key.p, d_key_s.p, d_iota.p, d_perm1.p, n, __builtin_ctzll(differ), bits_of(differ), st));
                perm = d_perm1.p;
                if (run_max) {
                    hipLaunchKernelGGL(k_collate_gather, grid_for(n), dim3(kCT), 0, st, n, (const uint32_t *)d_run[a].p,
                                       (const uint32_t *)d_perm1.p, d_run1.p);
                    OEM_HIP(hipGetLastError());
                    OEM_TRY(sort_pairs<uint32_t>(sc, d_run1.p, d_run1_s.p, d_perm1.p, d_perm2.p, n, 0, bits_of(run_max), st));
                    perm = d_perm2.p;
                }
            }
            hipLaunchKernelGGL(k_collate_recut, grid_for(n), dim3(kCT), 0, st, n, perm, (const uint64_t *)d_key.p,
                               (const uint32_t *)d_run[a].p, (const uint32_t *)d_ord[0].p, (const uint32_t *)d_pos[a].p,
                               (const uint8_t *)d_names.p, (const uint64_t *)d_off.p, off_base, round, d_order.p, d_head.p, d_ord[1].p,
                               d_flags.p, d_run1.p);
            OEM_HIP(hipGetLastError());
            OEM_TRY(scan_u64(sc, true, (const uint64_t *)d_flags.p, d_scan.p, n, st));
            OEM_HIP(hipMemsetAsync(d_run1_s.p, 0, sizeof(uint32_t) * n, st));
            hipLaunchKernelGGL(k_collate_mark, grid_for(n), dim3(kCT), 0, st, n, (const uint32_t *)d_run1.p, (const uint64_t *)d_scan.p,
                               d_run1_s.p);
            OEM_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_collate_keep, grid_for(n), dim3(kCT), 0, st, n, (const uint64_t *)d_scan.p, (const uint32_t *)d_run1_s.p,
                               d_flags.p);
            OEM_HIP(hipGetLastError());
            OEM_TRY(scan_u64(sc, true, (const uint64_t *)d_flags.p, d_scan.p, n, st));
            hipLaunchKernelGGL(k_collate_compact, grid_for(n), dim3(kCT), 0, st, n, (const uint64_t *)d_flags.p, (const uint64_t *)d_scan.p,
                               (const uint32_t *)d_pos[a].p, (const uint32_t *)d_ord[1].p, d_pos[a ^ 1].p, d_ord[0].p, d_run[a ^ 1].p);
            OEM_HIP(hipGetLastError());
            uint64_t total = 0;
            OEM_HIP(hipMemcpyAsync(&total, d_scan.p + (n - 1), sizeof total, hipMemcpyDeviceToHost, st));
            OEM_HIP(hipStreamSynchronize(st));
            a ^= 1;
            n = total & 0xffffffffull;
            if (!n) break;
            run_max = (total >> 32) - 1;
        }
        info[0] = std::max(info[0], (double)(round + 1));
        info[7] = std::max(info[7], (double)sorted_rounds);
    }
    if (cc.timing) OEM_HIP(hipEventRecord(ev[1].e, st));

    // the marks -> the batch's group_off (in d_key_s) and its cells' first groups
    {
        hipcub::TransformInputIterator<uint64_t, U32ToU64, const uint32_t *> in(d_head.p, U32ToU64());
        OEM_TRY(scan_u64(sc, false, in, d_scan.p, m + 1, st));
    }
    hipLaunchKernelGGL(k_collate_finish, grid_for(std::max<uint64_t>(m, nc + 1)), dim3(kCT), 0, st, m, nc, (const uint32_t *)d_head.p,
                       (const uint64_t *)d_scan.p, (const unsigned long long *)d_cell_off.p, order_base, pos_base, group_base, d_order.p,
                       d_key_s.p, d_cgo.p);
    OEM_HIP(hipGetLastError());
    if (cc.timing) OEM_HIP(hipEventRecord(ev[2].e, st));
    OEM_HIP(hipMemcpyAsync(&out->n_groups, d_scan.p + m, sizeof out->n_groups, hipMemcpyDeviceToHost, st));
    OEM_HIP(hipStreamSynchronize(st));
    if (cc.timing) {
        float t = 0.f;
        OEM_HIP(hipEventElapsedTime(&t, ev[0].e, ev[1].e));
        info[5] += t;
        OEM_HIP(hipEventElapsedTime(&t, ev[1].e, ev[2].e));
        info[5] += t;
    }
    std::swap(out->order.p, d_order.p);
    std::swap(out->group_off.p, d_key_s.p);
    std::swap(out->cell_group_off.p, d_cgo.p);
    return OEM_OK;
}

void launch_collate_validate(hipStream_t st, const uint8_t *d_names, uint64_t b0, uint64_t b1, const uint64_t *d_off, uint64_t r0,
                             uint64_t r1, unsigned long long *d_bad)
{
    const uint64_t words = b1 > b0 ? ((b1 + 15) >> 4) - (b0 >> 4) : 0;
    hipLaunchKernelGGL(k_collate_validate, grid_for(std::max(words, r1 - r0)), dim3(kCT), 0, st, d_names, b0, b1, d_off, (uint64_t)0, r0, r1,
                       (uint64_t)0, d_bad);
}

int gather_name_offsets(const uint32_t *d_order, uint64_t m, const uint64_t *d_name_off, uint64_t *d_out_off)
{
    Scratch sc;
    DevBuf<uint64_t> d_len;
    OEM_TRY(dev_alloc(&d_len.p, m + 1, nullptr));
    hipLaunchKernelGGL(k_names_lengths, grid_for(m + 1), dim3(kCT), 0, nullptr, m, d_order, d_name_off, d_len.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(scan_u64(sc, false, (const uint64_t *)d_len.p, d_out_off, m + 1, nullptr));
    OEM_HIP(hipStreamSynchronize(nullptr));
    return OEM_OK;
}

int gather_names(const uint32_t *d_order, uint64_t m, const uint8_t *d_names, const uint64_t *d_name_off, const uint64_t *d_out_off,
                 uint64_t off_base, uint64_t out_bytes, uint8_t *d_out, const uint8_t *d_sec, uint8_t *d_out_sec, bool with_empty)
{
    const uint64_t n_words = (out_bytes + 16) / 8; // the blob and its padding
    hipLaunchKernelGGL(k_names_gather, grid_for(n_words), dim3(kCT), 0, nullptr, n_words, out_bytes, m, d_order, d_names, d_name_off,
                       d_out_off, off_base, with_empty ? 1u : 0u, (uint64_t *)d_out);
    OEM_HIP(hipGetLastError());
    if (d_sec) {
        const uint64_t sec_words = (m + 1 + 7) / 8;
        hipLaunchKernelGGL(k_flags_gather, grid_for(sec_words), dim3(kCT), 0, nullptr, sec_words, m, d_order, d_sec, (uint64_t *)d_out_sec);
        OEM_HIP(hipGetLastError());
    }
    OEM_HIP(hipStreamSynchronize(nullptr));
    return OEM_OK;
}

namespace {

int cells_from_runs(uint64_t n, uint64_t n_runs, uint64_t n_input, const uint32_t *d_sorted, const uint64_t *d_run_off, bool timing,
                    double *cells_ms, BarcodeCells *out, DevBuf<uint32_t> *out_heads);

// The barcodes as one cell through the key rounds (cc: the host or the device form of the input), then the runs ranked by
// their first record and laid out in that rank.  out_heads (or NULL): the cells' first records, ascending.
int barcode_cells_of(CollateInput &cc, uint64_t n, bool timing, double *info, double *cells_ms, BarcodeCells *out,
                     DevBuf<uint32_t> *out_heads)
{
    const uint64_t one_cell[2] = {0, n};
    cc.what = "barcode";
    cc.cell_rec_off = one_cell;
    cc.mode = kCollateSort;
    cc.chunk_bytes = collate_chunk_bytes();
    cc.timing = timing;
    cc.cut_records = true;
    CollateResident cr; // order: the stable sort by barcode; group_off: where a barcode starts, closed by n
    OEM_TRY(collate_resident(cc, 0, 1, 0, 0, 0, info, &cr));
    return cells_from_runs(n, cr.n_groups, n, cr.order.p, cr.group_off.p, timing, cells_ms, out, out_heads);
}

// The runs of d_sorted (run_off: n_runs + 1 positions from 0, closed by n; the records are below n_input) ranked by their
// first record and laid out in that rank.
int cells_from_runs(uint64_t n, uint64_t n_runs, uint64_t n_input, const uint32_t *d_sorted, const uint64_t *d_run_off, bool timing,
                    double *cells_ms, BarcodeCells *out, DevBuf<uint32_t> *out_heads)
{
    Scratch sc;
    Event ev[2];
    if (timing)
        for (auto &e : ev) OEM_HIP(hipEventCreate(&e.e));
    DevBuf<uint32_t> d_head, d_head_s, d_idx, d_run_of_rank, d_rank_of_run, d_order_bc;
    DevBuf<uint64_t> d_len, d_cro;
    OEM_TRY(dev_alloc(&d_head.p, n_runs, nullptr));
    OEM_TRY(dev_alloc(&d_head_s.p, n_runs, nullptr));
    OEM_TRY(dev_alloc(&d_idx.p, n_runs, nullptr));
    OEM_TRY(dev_alloc(&d_run_of_rank.p, n_runs, nullptr));
    OEM_TRY(dev_alloc(&d_rank_of_run.p, n_runs, nullptr));
    OEM_TRY(dev_alloc(&d_order_bc.p, n, nullptr));
    OEM_TRY(dev_alloc(&d_len.p, n_runs + 1, nullptr));
    OEM_TRY(dev_alloc(&d_cro.p, n_runs + 1, nullptr));
    if (timing) OEM_HIP(hipEventRecord(ev[0].e, nullptr));
    hipLaunchKernelGGL(k_barcode_heads, grid_for(n_runs), dim3(kCT), 0, nullptr, n_runs, d_sorted,
                       d_run_off, d_head.p, d_idx.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(sort_pairs<uint32_t>(sc, d_head.p, d_head_s.p, d_idx.p, d_run_of_rank.p, n_runs, 0, std::max(bits_of(n_input - 1), 1), nullptr));
    hipLaunchKernelGGL(k_barcode_lengths, grid_for(n_runs + 1), dim3(kCT), 0, nullptr, n_runs, (const uint32_t *)d_run_of_rank.p,
                       d_run_off, d_len.p, d_rank_of_run.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(scan_u64(sc, false, (const uint64_t *)d_len.p, d_cro.p, n_runs + 1, nullptr));
    hipLaunchKernelGGL(k_barcode_scatter, grid_for(n), dim3(kCT), 0, nullptr, n, n_runs, d_sorted,
                       d_run_off, (const uint32_t *)d_rank_of_run.p, (const uint64_t *)d_cro.p, d_order_bc.p);
    OEM_HIP(hipGetLastError());
    if (timing) OEM_HIP(hipEventRecord(ev[1].e, nullptr));
    OEM_HIP(hipStreamSynchronize(nullptr));
    if (timing) {
        float t = 0.f;
        OEM_HIP(hipEventElapsedTime(&t, ev[0].e, ev[1].e));
        *cells_ms += t;
    }
    std::swap(out->order.p, d_order_bc.p);
    std::swap(out->cell_rec_off.p, d_cro.p);
    out->n_cells = n_runs;
    if (out_heads) std::swap(out_heads->p, d_head_s.p);
    return OEM_OK;
}

} // namespace

int collate_barcodes_resident(const char *who, const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n_records, bool timing,
                              double *info, double *cells_ms, BarcodeCells *out)
{
    CollateInput cc;
    cc.who = who;
    cc.names = barcodes;
    cc.name_off = barcode_off;
    return barcode_cells_of(cc, n_records, timing, info, cells_ms, out, nullptr);
}

int collate_barcodes_device(const char *who, const uint8_t *d_barcodes, const uint64_t *d_barcode_off, uint64_t n_bytes, uint64_t n_records,
                            BarcodeCells *out, DevBuf<uint32_t> *out_heads)
{
    CollateInput cc;
    cc.who = who;
    cc.d_names = d_barcodes;
    cc.d_name_off = d_barcode_off;
    cc.d_n_bytes = n_bytes;
    double info[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ms = 0;
    return barcode_cells_of(cc, n_records, false, info, &ms, out, out_heads);
}

int barcode_cells_from_runs(uint64_t n, uint64_t n_runs, uint64_t n_input, const uint32_t *d_sorted, const uint64_t *d_run_off,
                            BarcodeCells *out, DevBuf<uint32_t> *out_heads)
{
    double ms = 0;
    return cells_from_runs(n, n_runs, n_input, d_sorted, d_run_off, false, &ms, out, out_heads);
}

int check_barcode_input(const char *who, const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n_records)
{
    if (n_records > 0xffffffffull) return fail(OEM_ERR_ARG, "%s: %llu records: more than 2^32 - 1", who, (unsigned long long)n_records);
    if (n_records > kCollateMaxBatch)
        return fail(OEM_ERR_ARG, "%s: %llu records: the barcodes are sorted as one batch of at most 2^31 - 2", who, (unsigned long long)n_records);
    if (n_records && !barcodes) return fail(OEM_ERR_ARG, "%s: barcodes is NULL and n_records is not 0", who);
    return check_offsets(who, "barcode_off", barcode_off, n_records, "record");
}

namespace {

// One batch of oem_collate_names: the resident form, then its arrays to the caller's; *group_base counts the groups before
// the batch and is advanced.
int collate_batch(const CollateInput &cc, uint32_t c0, uint32_t c1, double *info, uint32_t *out_order, uint64_t *out_group_off,
                  uint64_t *out_cell_group_off, uint64_t *group_base)
{
    const uint64_t rec_base = cc.cell_rec_off[c0], m = cc.cell_rec_off[c1] - rec_base;
    CollateResident r;
    OEM_TRY(collate_resident(cc, c0, c1, rec_base, rec_base, *group_base, info, &r));
    OEM_HIP(hipMemcpy(out_order + rec_base, r.order.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    OEM_HIP(hipMemcpy(out_cell_group_off + c0, r.cell_group_off.p, sizeof(uint64_t) * ((size_t)(c1 - c0) + 1), hipMemcpyDeviceToHost));
    if (r.n_groups) OEM_HIP(hipMemcpy(out_group_off + *group_base, r.group_off.p, sizeof(uint64_t) * r.n_groups, hipMemcpyDeviceToHost));
    *group_base += r.n_groups;
    return OEM_OK;
}

} // namespace

uint64_t collate_chunk_bytes()
{
    const long ck = knob("OEM_COLLATE_CHUNK_BYTES", (long)kCollateChunkBytes);
    return ck > 0 ? (uint64_t)ck : kCollateChunkBytes;
}

uint64_t collate_batch_records()
{
    const long bk = knob("OEM_COLLATE_BATCH_RECORDS", (long)kCollateBatchRecords);
    return bk > 0 ? std::min<uint64_t>((uint64_t)bk, kCollateMaxBatch) : kCollateBatchRecords;
}

int check_collate_input(const char *who, const uint8_t *names, const uint64_t *name_off, uint64_t n_records, const uint64_t *cell_rec_off,
                        uint32_t n_cells, uint32_t mode)
{
    if (mode != OEM_COLLATE_SORT && mode != OEM_COLLATE_ADJACENT) return fail(OEM_ERR_ARG, "%s: mode %u is not a mode", who, mode);
    if (n_records > 0xffffffffull) return fail(OEM_ERR_ARG, "%s: %llu records: more than 2^32 - 1", who, (unsigned long long)n_records);
    if (n_records && !names) return fail(OEM_ERR_ARG, "%s: names is NULL and n_records is not 0", who);
    OEM_TRY(check_offsets(who, "name_off", name_off, n_records, "record"));
    OEM_TRY(check_offsets(who, "cell_rec_off", cell_rec_off, n_cells, "cell"));
    if (cell_rec_off[n_cells] != n_records)
        return fail(OEM_ERR_ARG, "%s: cell_rec_off ends at %llu, not at n_records = %llu", who, (unsigned long long)cell_rec_off[n_cells],
                    (unsigned long long)n_records);
    for (uint32_t c = 0; c < n_cells; ++c)
        if (cell_rec_off[c + 1] - cell_rec_off[c] > kCollateMaxBatch) return fail(OEM_ERR_ARG, "%s: cell %u has more than 2^31 - 2 records", who, c);
    return OEM_OK;
}

void collate_last_call(double *out8) { std::memcpy(out8, g_collate_last, sizeof g_collate_last); }
void collate_barcodes_last_call(double *out8) { std::memcpy(out8, g_barcodes_last, sizeof g_barcodes_last); }
void collate_barcodes_set_last(const double *in8) { std::memcpy(g_barcodes_last, in8, sizeof g_barcodes_last); }

} // namespace oem

using namespace oem;

extern "C" int oem_collate_names(const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary, uint64_t n_records,
                                 const uint64_t *cell_rec_off, uint32_t n_cells, uint32_t mode, int device, uint32_t *out_order,
                                 uint64_t *out_group_off, uint64_t *out_n_groups, uint64_t *out_cell_group_off)
{
    OEM_API_BEGIN
    if (!name_off || !cell_rec_off || !out_order || !out_group_off || !out_n_groups || !out_cell_group_off)
        return fail(OEM_ERR_ARG, "oem_collate_names: name_off, cell_rec_off or an output is NULL");
    OEM_TRY(check_collate_input("oem_collate_names", names, name_off, n_records, cell_rec_off, n_cells, mode));
    *out_n_groups = 0;
    OEM_TRY(ensure_device(device));

    CollateInput cc;
    cc.who = "oem_collate_names";
    cc.names = names;
    cc.name_off = name_off;
    cc.secondary = secondary;
    cc.cell_rec_off = cell_rec_off;
    cc.mode = mode;
    cc.chunk_bytes = collate_chunk_bytes();
    cc.timing = knob("OEM_COLLATE_TIMING", 0) != 0;
    double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t batch_records = collate_batch_records();
    std::memset(g_collate_last, 0, sizeof g_collate_last);

    uint64_t group_base = 0;
    out_cell_group_off[0] = 0;
    for (uint32_t c0 = 0; c0 < n_cells;) {
        uint32_t c1 = c0 + 1;
        while (c1 < n_cells && cell_rec_off[c1 + 1] - cell_rec_off[c0] <= batch_records) ++c1;
        if (cell_rec_off[c1] > cell_rec_off[c0]) {
            OEM_TRY(collate_batch(cc, c0, c1, info, out_order, out_group_off, out_cell_group_off, &group_base));
            info[2] += 1;
        } else {
            for (uint32_t c = c0; c <= c1; ++c) out_cell_group_off[c] = group_base;
        }
        c0 = c1;
    }
    out_group_off[group_base] = n_records;
    *out_n_groups = group_base;
    std::memcpy(g_collate_last, info, sizeof info);
    return OEM_OK;
    OEM_API_END("oem_collate_names")
}

extern "C" int oem_collate_barcodes(const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n_records, int device, uint32_t *out_order,
                                    uint64_t *out_cell_rec_off, uint64_t *out_n_cells)
{
    OEM_API_BEGIN
    const char *who = "oem_collate_barcodes";
    if (!barcode_off || !out_order || !out_cell_rec_off || !out_n_cells)
        return fail(OEM_ERR_ARG, "%s: barcode_off or an output is NULL", who);
    OEM_TRY(check_barcode_input(who, barcodes, barcode_off, n_records));
    *out_n_cells = 0;
    OEM_TRY(ensure_device(device));
    double info[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cells_ms = 0;
    std::memset(g_barcodes_last, 0, sizeof g_barcodes_last);
    out_cell_rec_off[0] = 0;
    if (n_records == 0) return OEM_OK;
    BarcodeCells bc;
    OEM_TRY(collate_barcodes_resident(who, barcodes, barcode_off, n_records, knob("OEM_COLLATE_TIMING", 0) != 0, info, &cells_ms, &bc));
    OEM_HIP(hipMemcpy(out_order, bc.order.p, sizeof(uint32_t) * n_records, hipMemcpyDeviceToHost));
    OEM_HIP(hipMemcpy(out_cell_rec_off, bc.cell_rec_off.p, sizeof(uint64_t) * (bc.n_cells + 1), hipMemcpyDeviceToHost));
    *out_n_cells = bc.n_cells;
    info[2] = cells_ms; // (no batches here: the slot holds the cells' kernels)
    std::memcpy(g_barcodes_last, info, sizeof info);
    return OEM_OK;
    OEM_API_END("oem_collate_barcodes")
}
