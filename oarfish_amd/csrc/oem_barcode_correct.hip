// oem_barcode_correct.hip -- oem_correct_barcodes: raw cell barcodes against a whitelist on the device, and the
// corrected stage that oem_em_run_cells_records_whitelist_sparse (oem_cells_records.hip) takes its cells from.  The rule
// and its host walk are oem_barcode_correct.h's; everything here is held to the walk exactly.
//
//   whitelist   the labels go up once as a padded blob; k_barcode_insert (oem_cells_barcodes_sort_stream.hip) puts every
//               label into the open-addressing table of oem_barcode_table.h, sized once at a load of at most 1/2.
//               k_wl_labels finds a label with a 0 byte before the insert, k_wl_distinct looks every label up behind it:
//               the smallest id among the labels equal to it must be its own.
//   exact       k_bc_exact, one record per lane: barcode_table_find, an integer atomicAdd on n(w) (exact in any order),
//               and the misses appended to a list with one atomic per wavefront (ballot, the leader adds the count, the
//               lanes take their ranks).  The list's order is arbitrary and nothing depends on it.  A barcode whose
//               length no label has is decided here: it has no neighbour.
//   neighbours  k_bc_neighbours, over the misses only and with n(w) complete: the lanes of a wavefront share one miss and
//               own its byte positions (a label is at most 64 bytes).  A lane computes the hash prefix up to its 8-byte
//               word once, tries the alphabet's bytes at its position (barcode_vote_position), and the 64 votes are
//               merged by an xor butterfly of shuffles; the merge commutes, so every lane holds the same vote and lane
//               0 stores the choice.
//   cells       the accepted records are compacted by a scan, (id, position) is sorted by one stable radix sort over the
//               bits W needs, the sorted ids' run starts are scanned into run offsets, and the runs are ranked by their
//               first record and laid out with the run kernels of collate_barcodes_device (barcode_cells_from_runs).
//   a session   (oem_cells_stream_set_whitelist; "The rule in a session" of the header): whitelist_batch runs k_bc_exact on a
//               batch's mapped records against the session's resident whitelist, whose n(w) is never reset, then
//               k_bc_neighbours_stream, which decides what does not depend on the counts and defers the rest, then
//               compacts the batch's survivor list to the retained records.  whitelist_finish runs the same kernel over
//               the pending list with the counts complete and scatters the winners' ids into the arena's id column;
//               barcode_cells_from_ids is the cells step above, shared by the one call and the session.
//
// No kernel both reads and writes the table; every probe loop ends after `capacity` steps with an error word.  The table
// of a 3 M-label whitelist is 32 MB of slots beside 48 MB of labels.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hipcub/hipcub.hpp>

#include "oem_barcode_correct.h"
#include "oem_cells_barcodes_stream.h"
#include "oem_collate_device.h"
#include "oem_parse_device.h"

namespace oem {
namespace {

constexpr int kBT = 256;
constexpr uint32_t kWave = 64;
inline dim3 grid_of(uint64_t n) { return dim3((unsigned)std::max<uint64_t>((n + kBT - 1) / kBT, 1)); }
inline int bits_of(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

enum : int { kBadLabel = 0, kBadPair = 1, kBadBarcode = 2, kBadTable = 3, kBadWords = 4 };

__device__ __forceinline__ uint64_t tid64() { return (uint64_t)blockIdx.x * kBT + threadIdx.x; }

// the smallest label that holds a 0 byte -> bad[kBadLabel]
__global__ __launch_bounds__(kBT) void k_wl_labels(uint64_t n_labels, const uint8_t *__restrict__ labels, const uint64_t *__restrict__ label_off,
                                                    unsigned long long *__restrict__ bad)
{
    const uint64_t w = tid64();
    if (w >= n_labels) return;
    const uint64_t l0 = label_off[w];
    if (barcode_has_zero_byte(labels + l0, label_off[w + 1] - l0)) atomicMin(bad + kBadLabel, (unsigned long long)w);
}

// every label looked up: the smallest id among the labels equal to label j is i; i < j is a pair of equal labels, and the
// smallest (i << 32 | j) -> bad[kBadPair]
__global__ __launch_bounds__(kBT) void k_wl_distinct(uint64_t n_labels, const uint32_t *__restrict__ slot, uint64_t capacity, uint32_t hash_bits,
                                                      const uint8_t *__restrict__ labels, const uint64_t *__restrict__ label_off,
                                                      unsigned long long *__restrict__ bad)
{
    const uint64_t j = tid64();
    if (j >= n_labels) return;
    const uint64_t l0 = label_off[j];
    const uint32_t i = barcode_table_find_smallest(slot, capacity, hash_bits, labels, label_off, labels + l0, label_off[j + 1] - l0);
    if (i == kBarcodeProbeError || i == kBarcodeEmpty || i > j) atomicOr(bad + kBadTable, 1ull);
    else if (i != j) atomicMin(bad + kBadPair, ((unsigned long long)i << 32) | (unsigned long long)j);
}

// One record per lane.  id / status of every record that is decided here (exact, missing, a length no label has), n(w),
// and the other records' indices appended to `miss`.  The smallest record whose barcode holds a 0 byte -> bad[kBadBarcode].
__global__ __launch_bounds__(kBT) void k_bc_exact(uint64_t n, const uint8_t *__restrict__ bc, const uint64_t *__restrict__ off,
                                                   const uint32_t *__restrict__ slot, uint64_t capacity, uint32_t hash_bits,
                                                   const uint8_t *__restrict__ labels, const uint64_t *__restrict__ label_off,
                                                   uint64_t n_labels, uint64_t len_mask, uint32_t *__restrict__ id, uint8_t *__restrict__ status,
                                                   uint32_t *__restrict__ count, uint32_t *__restrict__ miss, uint32_t *__restrict__ n_miss,
                                                   unsigned long long *__restrict__ bad)
{
    const uint64_t i = tid64();
    bool is_miss = false;
    if (i < n) {
        const uint64_t b0 = off[i], len = off[i + 1] - b0;
        uint32_t w = kBarcodeNoId;
        uint8_t st = kBarcodeMissing;
        if (len) {
            st = kBarcodeNoNeighbour;
            if (barcode_has_zero_byte(bc + b0, len)) {
                atomicMin(bad + kBadBarcode, (unsigned long long)i);
            } else if (len_mask & barcode_len_bit(len)) {
                uint64_t steps = 0;
                bool wrapped = false;
                const uint32_t f = barcode_table_find(slot, capacity, hash_bits, labels, label_off, bc + b0, len, &steps, &wrapped);
                if (f == kBarcodeEmpty) {
                    is_miss = true;
                } else if (f == kBarcodeProbeError || f >= n_labels) {
                    atomicOr(bad + kBadTable, 1ull);
                } else {
                    w = f;
                    st = kBarcodeExact;
                    atomicAdd(count + f, 1u);
                }
            }
        }
        id[i] = w;
        status[i] = st;
    }
    // the append, one atomic per wavefront: every lane of the wavefront arrives here
    const unsigned long long votes = __ballot(is_miss);
    if (votes) {
        const uint32_t lane = threadIdx.x & (kWave - 1u);
        const int leader = __ffsll((long long)votes) - 1;
        uint32_t first = 0;
        if ((int)lane == leader) first = atomicAdd(n_miss, (uint32_t)__popcll(votes));
        first = __shfl(first, leader, kWave);
        if (is_miss) miss[first + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
}

// The vote of the barcode p[0 .. len), 1 <= len <= 64, by one wavefront: a lane tries the alphabet's bytes at its byte
// position, and the 64 votes are merged by an xor butterfly of shuffles.  The merge commutes: every lane returns the
// same vote.  Every lane of the wavefront calls it.
__device__ __forceinline__ BarcodeVote wave_vote(uint32_t lane, const uint8_t *__restrict__ p, uint64_t len, const uint32_t *__restrict__ slot,
                                                 uint64_t capacity, uint32_t hash_bits, const uint8_t *__restrict__ labels,
                                                 const uint64_t *__restrict__ label_off, const uint32_t *__restrict__ count, uint64_t alphabet,
                                                 uint32_t n_alphabet, unsigned long long *__restrict__ bad)
{
    BarcodeVote v;
    uint64_t longest = 0;
    bool wrapped = false, broken = false;
    if (lane < len)
        barcode_vote_position(v, slot, capacity, hash_bits, labels, label_off, count, alphabet, n_alphabet, p, len, lane, &longest, &wrapped, &broken);
    if (broken) atomicOr(bad + kBadTable, 1ull);
    for (int d = (int)kWave / 2; d > 0; d >>= 1) {
        BarcodeVote o;
        o.found = __shfl_xor(v.found, d, kWave);
        o.best_n = __shfl_xor(v.best_n, d, kWave);
        o.n_best = __shfl_xor(v.n_best, d, kWave);
        o.id = __shfl_xor(v.id, d, kWave);
        barcode_vote_merge(v, o);
    }
    return v;
}

// One miss per wavefront, one byte position per lane (the misses' lengths are labels' lengths: 1 .. 64).
__global__ __launch_bounds__(kBT) void k_bc_neighbours(uint64_t n_miss, const uint32_t *__restrict__ miss, const uint8_t *__restrict__ bc,
                                                        const uint64_t *__restrict__ off, const uint32_t *__restrict__ slot, uint64_t capacity,
                                                        uint32_t hash_bits, const uint8_t *__restrict__ labels,
                                                        const uint64_t *__restrict__ label_off, const uint32_t *__restrict__ count,
                                                        uint64_t alphabet, uint32_t n_alphabet, uint32_t multi, uint32_t *__restrict__ id,
                                                        uint8_t *__restrict__ status, unsigned long long *__restrict__ bad)
{
    const uint64_t j = tid64() / kWave; // the same for every lane of a wavefront
    if (j >= n_miss) return;
    const uint32_t lane = threadIdx.x & (kWave - 1u);
    const uint64_t i = miss[j], b0 = off[i], len = off[i + 1] - b0;
    const BarcodeVote v = wave_vote(lane, bc + b0, len, slot, capacity, hash_bits, labels, label_off, count, alphabet, n_alphabet, bad);
    if (lane == 0) {
        uint32_t w = kBarcodeNoId;
        status[i] = barcode_vote_decide(v, multi, &w);
        id[i] = w;
    }
}

// The neighbour pass of a session ("The rule in a session", oem_barcode_correct.h), one item per wavefront as above.
//   per batch (at == NULL): miss[j] is a record of the batch's dense blob.  What does not depend on the counts is decided
//     -- a corrected record's id carries kBarcodeCorrectedBit --, the rest is kBarcodeDeferred and its record is appended
//     to `deferred` (capacity n_miss) by lane 0: one atomic per wavefront.  The list's order is arbitrary; its user sorts it.
//   finish (miss == NULL): item j of the pending blob, decided with the complete counts; status[j], and a winner's id to
//     id[at[j]], the arena's id column of n_id entries (a loser's stays kBarcodeNoId).
__global__ __launch_bounds__(kBT) void k_bc_neighbours_stream(uint64_t n_miss, const uint32_t *__restrict__ miss, const uint8_t *__restrict__ bc,
                                                               const uint64_t *__restrict__ off, const uint32_t *__restrict__ slot,
                                                               uint64_t capacity, uint32_t hash_bits, const uint8_t *__restrict__ labels,
                                                               const uint64_t *__restrict__ label_off, const uint32_t *__restrict__ count,
                                                               uint64_t alphabet, uint32_t n_alphabet, uint32_t multi,
                                                               const uint32_t *__restrict__ at, uint64_t n_id, uint32_t *__restrict__ id,
                                                               uint8_t *__restrict__ status, uint32_t *__restrict__ deferred,
                                                               uint32_t *__restrict__ n_deferred, unsigned long long *__restrict__ bad)
{
    const uint64_t j = tid64() / kWave;
    if (j >= n_miss) return;
    const uint32_t lane = threadIdx.x & (kWave - 1u);
    const uint64_t i = miss ? miss[j] : j, b0 = off[i], len = off[i + 1] - b0;
    const BarcodeVote v = wave_vote(lane, bc + b0, len, slot, capacity, hash_bits, labels, label_off, count, alphabet, n_alphabet, bad);
    if (lane != 0) return;
    uint32_t w = kBarcodeNoId;
    const uint8_t st = at ? barcode_vote_decide(v, multi, &w) : barcode_vote_decide_or_defer(v, multi, &w);
    if (st == kBarcodeCorrected) w |= kBarcodeCorrectedBit;
    status[i] = st;
    if (!at) {
        id[i] = w;
        if (st == kBarcodeDeferred) deferred[atomicAdd(n_deferred, 1u)] = (uint32_t)i;
    } else if (at[j] >= n_id) {
        atomicOr(bad + kBadTable, 1ull);
    } else if (st == kBarcodeCorrected) {
        id[at[j]] = w;
    }
}

// flag[k] = record k of a session's batch is retained (accepted or deferred); flag[m] = 0, for the scan
__global__ __launch_bounds__(kBT) void k_bc_retained(uint64_t m, const uint32_t *__restrict__ id, const uint8_t *__restrict__ status,
                                                      uint32_t *__restrict__ flag)
{
    const uint64_t k = tid64();
    if (k <= m) flag[k] = k < m && (id[k] != kBarcodeNoId || status[k] == kBarcodeDeferred) ? 1u : 0u;
}

// the retained records, dense and in batch order: their input indices and their ids
__global__ __launch_bounds__(kBT) void k_bc_retain_compact(uint64_t m, const uint32_t *__restrict__ flag, const uint64_t *__restrict__ at,
                                                            const uint32_t *__restrict__ order, const uint32_t *__restrict__ id,
                                                            uint32_t *__restrict__ ret_order, uint32_t *__restrict__ ret_id)
{
    const uint64_t k = tid64();
    if (k >= m || !flag[k]) return;
    ret_order[at[k]] = order[k];
    ret_id[at[k]] = id[k];
}

// pos[j] = base + the rank among the retained records of the deferred record deferred[j]
__global__ __launch_bounds__(kBT) void k_bc_deferred_pos(uint64_t n_def, const uint32_t *__restrict__ deferred, const uint64_t *__restrict__ at,
                                                          uint64_t base, uint32_t *__restrict__ pos)
{
    const uint64_t j = tid64();
    if (j < n_def) pos[j] = (uint32_t)(base + at[deferred[j]]);
}

// One cell per wavefront: its whitelist id (its first record's) and the number of its records that were corrected.
__global__ __launch_bounds__(kBT) void k_bc_cell_summary(uint64_t n_cells, const uint32_t *__restrict__ order, const uint64_t *__restrict__ cro,
                                                          const uint32_t *__restrict__ id, uint32_t *__restrict__ cell_label,
                                                          unsigned long long *__restrict__ cell_corrected)
{
    const uint64_t c = tid64() / kWave;
    if (c >= n_cells) return;
    const uint32_t lane = threadIdx.x & (kWave - 1u);
    const uint64_t p0 = cro[c], p1 = cro[c + 1];
    uint32_t cnt = 0; // (a cell holds fewer than 2^31 records)
    for (uint64_t p = p0 + lane; p < p1; p += kWave) cnt += id[order[p]] >> 31;
    for (int d = (int)kWave / 2; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, kWave);
    if (lane == 0) {
        cell_label[c] = id[order[p0]] & ~kBarcodeCorrectedBit;
        cell_corrected[c] = cnt;
    }
}

// flag[i] = record i is accepted; flag[n] = 0, for the scan
__global__ __launch_bounds__(kBT) void k_bc_accepted(uint64_t n, const uint32_t *__restrict__ id, uint32_t *__restrict__ flag)
{
    const uint64_t i = tid64();
    if (i <= n) flag[i] = i < n && id[i] != kBarcodeNoId ? 1u : 0u;
}

// the accepted records, dense and in input order: key = the label (id & mask: a session's ids carry kBarcodeCorrectedBit),
// val = the record
__global__ __launch_bounds__(kBT) void k_bc_compact(uint64_t n, const uint32_t *__restrict__ id, uint32_t mask, const uint64_t *__restrict__ at,
                                                     uint32_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const uint64_t i = tid64();
    if (i >= n || id[i] == kBarcodeNoId) return;
    key[at[i]] = id[i] & mask;
    val[at[i]] = (uint32_t)i;
}

// flag[p] = a run of equal keys starts at position p; flag[m] = 0
__global__ __launch_bounds__(kBT) void k_bc_run_flags(uint64_t m, const uint32_t *__restrict__ key, uint32_t *__restrict__ flag)
{
    const uint64_t p = tid64();
    if (p <= m) flag[p] = p < m && (p == 0 || key[p] != key[p - 1]) ? 1u : 0u;
}

// run_off[r] = the first position of run r; run_off[n_runs] = m
__global__ __launch_bounds__(kBT) void k_bc_run_off(uint64_t m, uint64_t n_runs, const uint32_t *__restrict__ flag, const uint64_t *__restrict__ at,
                                                     uint64_t *__restrict__ run_off)
{
    const uint64_t p = tid64();
    if (p > m) return;
    if (p == m) run_off[n_runs] = m;
    else if (flag[p]) run_off[at[p]] = p;
}

// counts[s] += the records of status s: a workgroup's tally in LDS, five atomics a workgroup
__global__ __launch_bounds__(kBT) void k_bc_tally(uint64_t n, const uint8_t *__restrict__ status, unsigned long long *__restrict__ counts)
{
    __shared__ uint32_t tally[kBarcodeStatuses];
    if (threadIdx.x < kBarcodeStatuses) tally[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = tid64();
    if (i < n && status[i] < kBarcodeStatuses) atomicAdd(&tally[status[i]], 1u);
    __syncthreads();
    if (threadIdx.x < kBarcodeStatuses && tally[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)tally[threadIdx.x]);
}

// the records order[0 .. m) of a resident blob: the smallest with a 0 byte -> bad[0], with no byte at all -> bad[1]
__global__ __launch_bounds__(kBT) void k_bc_validate_of(uint64_t m, const uint32_t *__restrict__ order, const uint8_t *__restrict__ blob,
                                                         const uint64_t *__restrict__ off, unsigned long long *__restrict__ bad)
{
    const uint64_t k = tid64();
    if (k >= m) return;
    const uint64_t i = order[k], b0 = off[i], len = off[i + 1] - b0;
    if (len == 0) atomicMin(bad + 1, (unsigned long long)i);
    else if (barcode_has_zero_byte(blob + b0, len)) atomicMin(bad + 0, (unsigned long long)i);
}

int sort_by_label(const uint32_t *key, uint32_t *key_s, const uint32_t *val, uint32_t *val_s, uint64_t m, int bits)
{
    DevBuf<uint8_t> tmp;
    size_t tb = 0;
    OEM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, key, key_s, val, val_s, (int)m, 0, bits, nullptr));
    OEM_TRY(dev_alloc(&tmp.p, tb, nullptr));
    OEM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, key, key_s, val, val_s, (int)m, 0, bits, nullptr));
    OEM_HIP(hipStreamSynchronize(nullptr));
    return OEM_OK;
}

} // namespace

int check_barcode_rule(const char *who, const oem_barcode_rule *rule)
{
    if (!rule) return fail(OEM_ERR_ARG, "%s: the barcode rule is NULL", who);
    uint64_t which = 0;
    const char *problem = barcode_rule_problem(rule->labels, rule->label_off, rule->n_labels, rule->multi, rule->alphabet, rule->n_alphabet, &which);
    if (!problem) return OEM_OK;
    char msg[160];
    std::snprintf(msg, sizeof msg, problem, (unsigned long long)which);
    return fail(OEM_ERR_ARG, "%s: %s", who, msg);
}

int whitelist_build(const char *who, const oem_barcode_rule *rule, BarcodeWhitelist *wl)
{
    static const uint8_t acgt[4] = {'A', 'C', 'G', 'T'};
    const uint8_t *alphabet = rule->alphabet ? rule->alphabet : acgt;
    wl->n_alphabet = rule->alphabet ? rule->n_alphabet : 4u;
    wl->alphabet = 0;
    for (uint32_t a = 0; a < wl->n_alphabet; ++a) wl->alphabet |= (uint64_t)alphabet[a] << (8 * a);
    wl->multi = rule->multi;
    const uint64_t W = rule->n_labels, n_bytes = rule->label_off[W];
    wl->n_labels = W;
    wl->len_mask = 0;
    for (uint64_t w = 0; w < W; ++w) wl->len_mask |= barcode_len_bit(rule->label_off[w + 1] - rule->label_off[w]);
    uint64_t cap = 2;
    const uint64_t slots0 = (uint64_t)std::max<long>(knob("OEM_BARCODE_TABLE_SLOTS0", (long)kBarcodeTableSlots0), 2);
    while (cap < slots0) cap *= 2;
    while (2 * W > cap) cap *= 2;
    wl->capacity = cap;
    wl->hash_bits = (uint32_t)std::min<long>(std::max<long>(knob("OEM_BARCODE_HASH_BITS", 64), 0), 64);

    OEM_TRY(dev_alloc(&wl->labels.p, n_bytes + 16, nullptr));
    OEM_TRY(dev_alloc(&wl->label_off.p, W + 1, nullptr));
    OEM_TRY(dev_alloc(&wl->slot.p, cap, nullptr));
    OEM_TRY(dev_alloc(&wl->count.p, W, nullptr));
    OEM_TRY(dev_alloc(&wl->bad.p, kBadWords, nullptr));
    OEM_HIP(hipMemcpy(wl->labels.p, rule->labels, n_bytes, hipMemcpyHostToDevice));
    OEM_HIP(hipMemset(wl->labels.p + n_bytes, 0, 16));
    OEM_HIP(hipMemcpy(wl->label_off.p, rule->label_off, sizeof(uint64_t) * (W + 1), hipMemcpyHostToDevice));
    OEM_HIP(hipMemset(wl->slot.p, 0xff, sizeof(uint32_t) * cap));
    OEM_HIP(hipMemset(wl->count.p, 0, sizeof(uint32_t) * W));
    const unsigned long long bad0[kBadWords] = {~0ull, ~0ull, ~0ull, 0ull};
    OEM_HIP(hipMemcpy(wl->bad.p, bad0, sizeof bad0, hipMemcpyHostToDevice));

    unsigned long long bad[kBadWords];
    hipLaunchKernelGGL(k_wl_labels, grid_of(W), dim3(kBT), 0, nullptr, W, (const uint8_t *)wl->labels.p, (const uint64_t *)wl->label_off.p, wl->bad.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpy(bad, wl->bad.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[kBadLabel] != ~0ull) return fail(OEM_ERR_ARG, "%s: label %llu of the whitelist contains a 0 byte", who, bad[kBadLabel]);
    DevBuf<unsigned long long> d_stats; // k_barcode_insert's words: the longest probe, a probe wrapped, an error
    OEM_TRY(dev_alloc(&d_stats.p, 3, nullptr));
    OEM_HIP(hipMemset(d_stats.p, 0, sizeof(unsigned long long) * 3));
    OEM_TRY(barcode_table_insert(0, W, wl->slot.p, cap, wl->hash_bits, wl->labels.p, wl->label_off.p, d_stats.p));
    hipLaunchKernelGGL(k_wl_distinct, grid_of(W), dim3(kBT), 0, nullptr, W, (const uint32_t *)wl->slot.p, cap, wl->hash_bits,
                       (const uint8_t *)wl->labels.p, (const uint64_t *)wl->label_off.p, wl->bad.p);
    OEM_HIP(hipGetLastError());
    unsigned long long stats[3];
    OEM_HIP(hipMemcpy(stats, d_stats.p, sizeof stats, hipMemcpyDeviceToHost));
    OEM_HIP(hipMemcpy(bad, wl->bad.p, sizeof bad, hipMemcpyDeviceToHost));
    if (stats[2] || bad[kBadTable])
        return fail(OEM_ERR_STATE, "%s: the whitelist table is broken: a probe went round all %llu slots, or a label was not found after its insert",
                    who, (unsigned long long)cap);
    if (bad[kBadPair] != ~0ull)
        return fail(OEM_ERR_ARG, "%s: labels %llu and %llu of the whitelist are equal", who, bad[kBadPair] >> 32, bad[kBadPair] & 0xffffffffull);
    return OEM_OK;
}

int correct_barcodes_resident(const char *who, const BarcodeWhitelist &wl, const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n,
                              CorrectedCells *out)
{
    out->n_accepted = 0;
    out->n_misses = 0;
    out->cells.n_cells = 0;
    std::fill(out->counts, out->counts + kBarcodeStatuses, 0ull);
    if (n == 0) return OEM_OK;
    OEM_TRY(dev_alloc(&out->id.p, n, nullptr));
    OEM_TRY(dev_alloc(&out->status.p, n, nullptr));
    DevBuf<unsigned long long> d_counts;
    OEM_TRY(dev_alloc(&d_counts.p, kBarcodeStatuses, nullptr));
    OEM_HIP(hipMemset(d_counts.p, 0, sizeof(unsigned long long) * kBarcodeStatuses));
    {
        // the barcodes up through the upload lanes, as the UMIs go (an empty one is legal); they are checked by k_bc_exact
        DevBuf<uint8_t> d_bc;
        DevBuf<uint64_t> d_bc_off;
        DevBuf<uint32_t> d_miss, d_n_miss;
        OEM_TRY(umis_upload(who, barcodes, barcode_off, n, &d_bc, &d_bc_off, false));
        OEM_TRY(dev_alloc(&d_miss.p, n, nullptr));
        OEM_TRY(dev_alloc(&d_n_miss.p, 1, nullptr));
        OEM_HIP(hipMemset(d_n_miss.p, 0, sizeof(uint32_t)));
        hipLaunchKernelGGL(k_bc_exact, grid_of(n), dim3(kBT), 0, nullptr, n, (const uint8_t *)d_bc.p, (const uint64_t *)d_bc_off.p,
                           (const uint32_t *)wl.slot.p, wl.capacity, wl.hash_bits, (const uint8_t *)wl.labels.p, (const uint64_t *)wl.label_off.p,
                           wl.n_labels, wl.len_mask, out->id.p, out->status.p, wl.count.p, d_miss.p, d_n_miss.p, wl.bad.p);
        OEM_HIP(hipGetLastError());
        uint32_t n_miss = 0;
        unsigned long long bad[kBadWords];
        OEM_HIP(hipMemcpy(&n_miss, d_n_miss.p, sizeof n_miss, hipMemcpyDeviceToHost));
        OEM_HIP(hipMemcpy(bad, wl.bad.p, sizeof bad, hipMemcpyDeviceToHost));
        if (bad[kBadBarcode] != ~0ull) return fail(OEM_ERR_ARG, "%s: the barcode of record %llu contains a 0 byte", who, bad[kBadBarcode]);
        if (n_miss > n) return fail(OEM_ERR_STATE, "%s: %u misses among %llu records", who, n_miss, (unsigned long long)n);
        out->n_misses = n_miss;
        if (n_miss) {
            hipLaunchKernelGGL(k_bc_neighbours, grid_of((uint64_t)n_miss * kWave), dim3(kBT), 0, nullptr, (uint64_t)n_miss, (const uint32_t *)d_miss.p,
                               (const uint8_t *)d_bc.p, (const uint64_t *)d_bc_off.p, (const uint32_t *)wl.slot.p, wl.capacity, wl.hash_bits,
                               (const uint8_t *)wl.labels.p, (const uint64_t *)wl.label_off.p, (const uint32_t *)wl.count.p, wl.alphabet,
                               wl.n_alphabet, wl.multi, out->id.p, out->status.p, wl.bad.p);
            OEM_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(k_bc_tally, grid_of(n), dim3(kBT), 0, nullptr, n, (const uint8_t *)out->status.p, d_counts.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpy(bad, wl.bad.p, sizeof bad, hipMemcpyDeviceToHost));
        if (bad[kBadTable])
            return fail(OEM_ERR_STATE, "%s: the whitelist table is broken: a probe went round all %llu slots", who, (unsigned long long)wl.capacity);
        unsigned long long counts[kBarcodeStatuses];
        OEM_HIP(hipMemcpy(counts, d_counts.p, sizeof counts, hipMemcpyDeviceToHost));
        std::copy(counts, counts + kBarcodeStatuses, out->counts);
    }

    // the cells of the accepted records
    const uint64_t m = out->counts[kBarcodeExact] + out->counts[kBarcodeCorrected];
    out->n_accepted = m;
    if (m == 0) return OEM_OK;
    uint64_t m_scan = 0;
    return barcode_cells_from_ids(who, out->id.p, ~0u, n, wl.n_labels, m, &out->cells, &m_scan);
}

int barcode_cells_from_ids(const char *who, const uint32_t *d_id, uint32_t mask, uint64_t n, uint64_t n_labels, uint64_t m_expected,
                           BarcodeCells *cells, uint64_t *n_accepted)
{
    cells->n_cells = 0;
    *n_accepted = 0;
    if (n == 0) return OEM_OK;
    DevBuf<uint32_t> d_flag, d_key, d_val, d_key_s, d_val_s;
    DevBuf<uint64_t> d_at, d_run_off;
    OEM_TRY(dev_alloc(&d_flag.p, n + 1, nullptr));
    OEM_TRY(dev_alloc(&d_at.p, n + 1, nullptr));
    hipLaunchKernelGGL(k_bc_accepted, grid_of(n + 1), dim3(kBT), 0, nullptr, n, d_id, d_flag.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(exclusive_scan_u32(d_flag.p, d_at.p, n + 1));
    uint64_t m = 0;
    OEM_HIP(hipMemcpy(&m, d_at.p + n, sizeof m, hipMemcpyDeviceToHost));
    if (m_expected != kBarcodeNoIndex && m != m_expected)
        return fail(OEM_ERR_STATE, "%s: %llu records have a label and %llu are exact or corrected", who, (unsigned long long)m,
                    (unsigned long long)m_expected);
    *n_accepted = m;
    if (m == 0) return OEM_OK;
    OEM_TRY(dev_alloc(&d_key.p, m, nullptr));
    OEM_TRY(dev_alloc(&d_val.p, m, nullptr));
    OEM_TRY(dev_alloc(&d_key_s.p, m, nullptr));
    OEM_TRY(dev_alloc(&d_val_s.p, m, nullptr));
    hipLaunchKernelGGL(k_bc_compact, grid_of(n), dim3(kBT), 0, nullptr, n, d_id, mask, (const uint64_t *)d_at.p, d_key.p, d_val.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(sort_by_label(d_key.p, d_key_s.p, d_val.p, d_val_s.p, m, std::max(bits_of(n_labels - 1), 1)));
    d_key.reset();
    d_val.reset();
    hipLaunchKernelGGL(k_bc_run_flags, grid_of(m + 1), dim3(kBT), 0, nullptr, m, (const uint32_t *)d_key_s.p, d_flag.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(exclusive_scan_u32(d_flag.p, d_at.p, m + 1));
    uint64_t n_runs = 0;
    OEM_HIP(hipMemcpy(&n_runs, d_at.p + m, sizeof n_runs, hipMemcpyDeviceToHost));
    if (n_runs == 0 || n_runs > m || n_runs > n_labels)
        return fail(OEM_ERR_STATE, "%s: %llu accepted records gave %llu cells", who, (unsigned long long)m, (unsigned long long)n_runs);
    OEM_TRY(dev_alloc(&d_run_off.p, n_runs + 1, nullptr));
    hipLaunchKernelGGL(k_bc_run_off, grid_of(m + 1), dim3(kBT), 0, nullptr, m, n_runs, (const uint32_t *)d_flag.p, (const uint64_t *)d_at.p,
                       d_run_off.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipStreamSynchronize(nullptr));
    d_flag.reset();
    d_at.reset();
    d_key_s.reset();
    return barcode_cells_from_runs(m, n_runs, n, d_val_s.p, d_run_off.p, cells, nullptr);
}

// ---- the rule in a session (oem_barcode_correct.h): a batch, the pending pass at finish, the cells' summary

int whitelist_batch(const char *who, const BarcodeWhitelist &wl, const uint8_t *d_bc, const uint64_t *d_bc_off, const uint32_t *d_order, uint64_t m,
                    uint64_t arena_n, WhitelistBatch *out)
{
    out->n_retained = out->n_deferred = 0;
    std::fill(out->counts, out->counts + kBarcodeStatuses, 0ull);
    if (m == 0) return OEM_OK;
    DevBuf<uint32_t> d_id, d_miss, d_n, d_flag, d_def;
    DevBuf<uint8_t> d_status;
    DevBuf<uint64_t> d_at;
    DevBuf<unsigned long long> d_counts;
    OEM_TRY(dev_alloc(&d_id.p, m, nullptr));
    OEM_TRY(dev_alloc(&d_status.p, m, nullptr));
    OEM_TRY(dev_alloc(&d_miss.p, m, nullptr));
    OEM_TRY(dev_alloc(&d_n.p, 2, nullptr)); // the misses, the deferred
    OEM_TRY(dev_alloc(&d_counts.p, kBarcodeStatuses, nullptr));
    OEM_HIP(hipMemset(d_n.p, 0, sizeof(uint32_t) * 2));
    OEM_HIP(hipMemset(d_counts.p, 0, sizeof(unsigned long long) * kBarcodeStatuses));
    hipLaunchKernelGGL(k_bc_exact, grid_of(m), dim3(kBT), 0, nullptr, m, d_bc, d_bc_off, (const uint32_t *)wl.slot.p, wl.capacity, wl.hash_bits,
                       (const uint8_t *)wl.labels.p, (const uint64_t *)wl.label_off.p, wl.n_labels, wl.len_mask, d_id.p, d_status.p, wl.count.p,
                       d_miss.p, d_n.p, wl.bad.p);
    OEM_HIP(hipGetLastError());
    uint32_t cnt[2] = {0, 0};
    unsigned long long bad[kBadWords];
    OEM_HIP(hipMemcpy(cnt, d_n.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    OEM_HIP(hipMemcpy(bad, wl.bad.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[kBadBarcode] != ~0ull) // (the caller has checked the blob: not reached)
        return fail(OEM_ERR_STATE, "%s: a barcode with a 0 byte reached the exact pass", who);
    const uint64_t n_miss = cnt[0];
    if (n_miss > m) return fail(OEM_ERR_STATE, "%s: %llu misses among %llu records", who, (unsigned long long)n_miss, (unsigned long long)m);
    if (n_miss) {
        OEM_TRY(dev_alloc(&d_def.p, n_miss, nullptr));
        hipLaunchKernelGGL(k_bc_neighbours_stream, grid_of(n_miss * kWave), dim3(kBT), 0, nullptr, n_miss, (const uint32_t *)d_miss.p, d_bc, d_bc_off,
                           (const uint32_t *)wl.slot.p, wl.capacity, wl.hash_bits, (const uint8_t *)wl.labels.p, (const uint64_t *)wl.label_off.p,
                           (const uint32_t *)wl.count.p, wl.alphabet, wl.n_alphabet, wl.multi, (const uint32_t *)nullptr, m, d_id.p, d_status.p,
                           d_def.p, d_n.p + 1, wl.bad.p);
        OEM_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_bc_tally, grid_of(m), dim3(kBT), 0, nullptr, m, (const uint8_t *)d_status.p, d_counts.p); // (a deferred record: in none)
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpy(cnt, d_n.p, sizeof cnt, hipMemcpyDeviceToHost));
    OEM_HIP(hipMemcpy(bad, wl.bad.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[kBadTable])
        return fail(OEM_ERR_STATE, "%s: the whitelist table is broken: a probe went round all %llu slots", who, (unsigned long long)wl.capacity);
    unsigned long long counts[kBarcodeStatuses];
    OEM_HIP(hipMemcpy(counts, d_counts.p, sizeof counts, hipMemcpyDeviceToHost));
    std::copy(counts, counts + kBarcodeStatuses, out->counts);
    const uint64_t n_def = cnt[1];
    if (n_def > n_miss) return fail(OEM_ERR_STATE, "%s: %llu deferred among %llu misses", who, (unsigned long long)n_def, (unsigned long long)n_miss);
    d_miss.reset();

    // the retained records: the batch's survivor list and the ids, compacted to them
    OEM_TRY(dev_alloc(&d_flag.p, m + 1, nullptr));
    OEM_TRY(dev_alloc(&d_at.p, m + 1, nullptr));
    hipLaunchKernelGGL(k_bc_retained, grid_of(m + 1), dim3(kBT), 0, nullptr, m, (const uint32_t *)d_id.p, (const uint8_t *)d_status.p, d_flag.p);
    OEM_HIP(hipGetLastError());
    OEM_TRY(exclusive_scan_u32(d_flag.p, d_at.p, m + 1));
    uint64_t n_ret = 0;
    OEM_HIP(hipMemcpy(&n_ret, d_at.p + m, sizeof n_ret, hipMemcpyDeviceToHost));
    if (n_ret != counts[kBarcodeExact] + counts[kBarcodeCorrected] + n_def)
        return fail(OEM_ERR_STATE, "%s: %llu records are retained, %llu are accepted or deferred", who, (unsigned long long)n_ret,
                    (unsigned long long)(counts[kBarcodeExact] + counts[kBarcodeCorrected] + n_def));
    out->n_retained = n_ret;
    out->n_deferred = n_def;
    if (n_ret == 0) return OEM_OK;
    OEM_TRY(dev_alloc(&out->order.p, n_ret, nullptr));
    OEM_TRY(dev_alloc(&out->id.p, n_ret, nullptr));
    hipLaunchKernelGGL(k_bc_retain_compact, grid_of(m), dim3(kBT), 0, nullptr, m, (const uint32_t *)d_flag.p, (const uint64_t *)d_at.p, d_order,
                       (const uint32_t *)d_id.p, out->order.p, out->id.p);
    OEM_HIP(hipGetLastError());
    if (n_def) {
        // the deferred records in batch order, whatever order the atomics gave them: their barcodes and arena positions
        DevBuf<uint32_t> d_def_s;
        DevBuf<uint8_t> tmp;
        size_t tb = 0;
        const int bits = std::max(bits_of(m - 1), 1);
        OEM_TRY(dev_alloc(&d_def_s.p, n_def, nullptr));
        OEM_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, (const uint32_t *)d_def.p, d_def_s.p, (int)n_def, 0, bits, nullptr));
        OEM_TRY(dev_alloc(&tmp.p, tb, nullptr));
        OEM_HIP(hipcub::DeviceRadixSort::SortKeys(tmp.p, tb, (const uint32_t *)d_def.p, d_def_s.p, (int)n_def, 0, bits, nullptr));
        OEM_TRY(dev_alloc(&out->deferred_pos.p, n_def, nullptr));
        hipLaunchKernelGGL(k_bc_deferred_pos, grid_of(n_def), dim3(kBT), 0, nullptr, n_def, (const uint32_t *)d_def_s.p, (const uint64_t *)d_at.p,
                           arena_n, out->deferred_pos.p);
        OEM_HIP(hipGetLastError());
        OEM_TRY(gather_input_names(d_def_s.p, n_def, d_bc, d_bc_off, &out->deferred_off, &out->deferred_bc, &out->deferred_bytes));
    }
    OEM_HIP(hipStreamSynchronize(nullptr));
    return OEM_OK;
}

int whitelist_finish(const char *who, const BarcodeWhitelist &wl, const uint8_t *d_pending, const uint64_t *d_pending_off,
                     const uint32_t *d_pending_pos, uint64_t n_pending, uint32_t *d_arena_id, uint64_t arena_n, uint64_t *counts)
{
    std::fill(counts, counts + kBarcodeStatuses, 0ull);
    if (n_pending == 0) return OEM_OK;
    DevBuf<uint8_t> d_status;
    DevBuf<unsigned long long> d_counts;
    OEM_TRY(dev_alloc(&d_status.p, n_pending, nullptr));
    OEM_TRY(dev_alloc(&d_counts.p, kBarcodeStatuses, nullptr));
    OEM_HIP(hipMemset(d_counts.p, 0, sizeof(unsigned long long) * kBarcodeStatuses));
    hipLaunchKernelGGL(k_bc_neighbours_stream, grid_of(n_pending * kWave), dim3(kBT), 0, nullptr, n_pending, (const uint32_t *)nullptr, d_pending,
                       d_pending_off, (const uint32_t *)wl.slot.p, wl.capacity, wl.hash_bits, (const uint8_t *)wl.labels.p,
                       (const uint64_t *)wl.label_off.p, (const uint32_t *)wl.count.p, wl.alphabet, wl.n_alphabet, wl.multi, d_pending_pos, arena_n,
                       d_arena_id, d_status.p, (uint32_t *)nullptr, (uint32_t *)nullptr, wl.bad.p);
    OEM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_bc_tally, grid_of(n_pending), dim3(kBT), 0, nullptr, n_pending, (const uint8_t *)d_status.p, d_counts.p);
    OEM_HIP(hipGetLastError());
    unsigned long long bad[kBadWords], c[kBarcodeStatuses];
    OEM_HIP(hipMemcpy(bad, wl.bad.p, sizeof bad, hipMemcpyDeviceToHost));
    OEM_HIP(hipMemcpy(c, d_counts.p, sizeof c, hipMemcpyDeviceToHost));
    if (bad[kBadTable])
        return fail(OEM_ERR_STATE, "%s: the whitelist table is broken: a probe went round all %llu slots, or a pending record lies outside the arena",
                    who, (unsigned long long)wl.capacity);
    std::copy(c, c + kBarcodeStatuses, counts);
    return OEM_OK;
}

int whitelist_cell_summary(const BarcodeCells &cells, const uint32_t *d_arena_id, std::vector<uint32_t> *cell_label,
                           std::vector<uint64_t> *cell_corrected)
{
    const uint64_t nc = cells.n_cells;
    cell_label->assign(nc, 0);
    cell_corrected->assign(nc, 0);
    if (nc == 0) return OEM_OK;
    DevBuf<uint32_t> d_label;
    DevBuf<unsigned long long> d_corr;
    OEM_TRY(dev_alloc(&d_label.p, nc, nullptr));
    OEM_TRY(dev_alloc(&d_corr.p, nc, nullptr));
    hipLaunchKernelGGL(k_bc_cell_summary, grid_of(nc * kWave), dim3(kBT), 0, nullptr, nc, (const uint32_t *)cells.order.p,
                       (const uint64_t *)cells.cell_rec_off.p, d_arena_id, d_label.p, d_corr.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpy(cell_label->data(), d_label.p, sizeof(uint32_t) * nc, hipMemcpyDeviceToHost));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counts come down as they are");
    OEM_HIP(hipMemcpy(cell_corrected->data(), d_corr.p, sizeof(uint64_t) * nc, hipMemcpyDeviceToHost));
    return OEM_OK;
}

int validate_records_of(const uint32_t *d_order, uint64_t m, const uint8_t *d_blob, const uint64_t *d_off, unsigned long long *bad2)
{
    bad2[0] = bad2[1] = ~0ull;
    if (m == 0) return OEM_OK;
    DevBuf<unsigned long long> d_bad;
    OEM_TRY(dev_alloc(&d_bad.p, 2, nullptr));
    OEM_HIP(hipMemcpy(d_bad.p, bad2, sizeof(unsigned long long) * 2, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_bc_validate_of, grid_of(m), dim3(kBT), 0, nullptr, m, d_order, d_blob, d_off, d_bad.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpy(bad2, d_bad.p, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost));
    return OEM_OK;
}

} // namespace oem

using namespace oem;

extern "C" int oem_correct_barcodes(const oem_barcode_rule *rule, const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n_records,
                                    int device, uint32_t *out_id, uint8_t *out_status, uint32_t *out_order, uint64_t *out_cell_rec_off,
                                    uint64_t *out_n_cells, uint64_t *out_n_accepted, uint64_t *out_counts)
{
    OEM_API_BEGIN
    const char *who = "oem_correct_barcodes";
    if (!barcode_off || !out_n_cells || !out_n_accepted) return fail(OEM_ERR_ARG, "%s: barcode_off, out_n_cells or out_n_accepted is NULL", who);
    *out_n_cells = 0;
    *out_n_accepted = 0;
    OEM_TRY(check_barcode_rule(who, rule));
    OEM_TRY(check_barcode_input(who, barcodes, barcode_off, n_records));
    OEM_TRY(ensure_device(device));
    BarcodeWhitelist wl;
    OEM_TRY(whitelist_build(who, rule, &wl));
    CorrectedCells cc;
    OEM_TRY(correct_barcodes_resident(who, wl, barcodes, barcode_off, n_records, &cc));
    const uint64_t n = n_records, m = cc.n_accepted, nc = cc.cells.n_cells;
    if (out_id && n) OEM_HIP(hipMemcpy(out_id, cc.id.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    if (out_status && n) OEM_HIP(hipMemcpy(out_status, cc.status.p, n, hipMemcpyDeviceToHost));
    if (out_order && m) OEM_HIP(hipMemcpy(out_order, cc.cells.order.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    if (out_cell_rec_off) {
        out_cell_rec_off[0] = 0;
        if (nc) OEM_HIP(hipMemcpy(out_cell_rec_off, cc.cells.cell_rec_off.p, sizeof(uint64_t) * (nc + 1), hipMemcpyDeviceToHost));
    }
    if (out_counts) std::copy(cc.counts, cc.counts + kBarcodeStatuses, out_counts);
    *out_n_cells = nc;
    *out_n_accepted = m;
    return OEM_OK;
    OEM_API_END("oem_correct_barcodes")
}
