// oem_records_names.hip -- oem_store_create_records_names: the bulk parser (alignment_parser.rs:301-437, parse_alignments)
// and oem_store_create_records joined on the device.  Records, read names and secondary flags come in the caller's input
// order; the rule is oem_collate.h's (the bulk parser).  In this order, everything on the null stream unless said:
//
//   upload     records, names, offsets and flags once, in input order, through the pinned lanes of oem_filter_device.h
//   survivors  k_parse_keep takes the survivor mask from the records' flags (a record is five aligned words; its flags
//              are the low half of the fifth), one hipcub scan and k_parse_compact write order_parse, the surviving
//              input indices in ascending order.  Without an unmapped record order_parse is the identity and none of
//              the next step's gathers runs: the input blob is used where it is
//   names      gather_name_offsets, k_names_gather and k_flags_gather (oem_collate_device.hip) over order_parse build the
//              dense names and flags of the survivors, and k_collate_validate runs on that blob, so the name of a
//              skipped record is never examined; a bad name is mapped back through order_parse for the message.  The
//              gather walks names of at least a byte, so the empty names are found first, from the offsets alone, and
//              only the survivors before the first of them are gathered and searched for a 0 byte
//   collate    collate_resident in its device form over the survivors as one cell; k_order_compose turns its positions
//              into input indices.  Under OEM_COLLATE_ADJACENT with no unmapped record nothing is sorted or moved
//   check      k_parse_heads takes the first record of each of the first min(N, n_groups) groups; their names are
//              gathered and sorted as one cell by the same collate_resident (stable, no flags: a run of one name holds
//              its groups in ascending order).  k_parse_check takes the minimum, over the runs longer than one, of the
//              run's second group, packed with the run's first group
//   gather     k_records_gather through the composed order (not under ADJACENT without an unmapped record)
//   filter     filter_device_resident with the whole batch as one cell, then, before the store takes the arrays,
//              k_parse_unique (a wavefront sum and one atomic per wavefront over n_kept) and the row names:
//              k_parse_row_heads puts the first record of every kept group at the group's row, and the same name
//              gather writes the rows' names
//   store      filter_result_to_store, with the coverage model first when there is one
//
// Everything from `collate` on is parse_tail (oem_parse_device.h): the sorting names session's finish
// (oem_records_stream.hip) runs it on its arena of survivors, as this call runs it on its uploaded input.
//
// The host loop takes the groups when the filter would (no gap table for score_prob_denom, a score beyond +-2^24): order
// and group_off come down, the records are gathered on the host and go through add_groups_host; the result is the same.
//
// Device memory: 40 B a record, the names and 8 B a record of offsets are resident until the filter has run (the
// records twice for the length of their gather); order_parse adds 4 B a record, the survivor scan 12 B a record while
// it runs, and the collation about 150 B a surviving record while it runs, released before the records are gathered.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "oem_dev_blob.h"
#include "oem_parse_device.h"

namespace oem {
namespace {

constexpr int kPT = 256;
static_assert(kRecUnmapped == OEM_REC_UNMAPPED, "oem_collate.h's bulk rule reads OEM_REC_UNMAPPED");
static_assert(sizeof(oem_aln_record) == 40 && offsetof(oem_aln_record, flags) == 32, "flags: the low half of a record's fifth word");

thread_local double g_records_names_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};

struct U32ToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};
struct NonZeroToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v ? 1 : 0; }
};

inline dim3 grid_for(uint64_t n) { return dim3((unsigned)std::max<uint64_t>((n + kPT - 1) / kPT, 1)); }

// keep[i] = record i is not unmapped, for i < n; keep[n] = 0 (the scan reads n + 1 entries)
__global__ __launch_bounds__(kPT) void k_parse_keep(uint64_t n, const uint64_t *__restrict__ rec_words, uint32_t *__restrict__ keep)
{
    const uint64_t i = (uint64_t)blockIdx.x * kPT + threadIdx.x;
    if (i > n) return;
    keep[i] = i < n ? (uint32_t)(((uint32_t)rec_words[i * 5 + 4] & kRecUnmapped) == 0) : 0u;
}

// order_parse[at[i]] = i for the survivors: at is the exclusive scan of keep
__global__ __launch_bounds__(kPT) void k_parse_compact(uint64_t n, const uint32_t *__restrict__ keep, const uint64_t *__restrict__ at,
                                                        uint32_t *__restrict__ order_parse)
{
    const uint64_t i = (uint64_t)blockIdx.x * kPT + threadIdx.x;
    if (i < n && keep[i]) order_parse[at[i]] = (uint32_t)i;
}

// heads[g] = the input index of the first record of group g, for g < n
__global__ __launch_bounds__(kPT) void k_parse_heads(uint64_t n, const uint64_t *__restrict__ group_off, const uint32_t *__restrict__ order,
                                                      uint32_t *__restrict__ heads)
{
    const uint64_t g = (uint64_t)blockIdx.x * kPT + threadIdx.x;
    if (g < n) heads[g] = order[group_off[g]];
}

// One lane per run of one name among the checked groups (run_off: n_runs + 1 positions of `sorted`, which holds group
// indices, ascending inside a run): a run longer than one is a repeated name, its second member the first group to
// repeat it.  *found = min over such runs of (second << 32 | first).
__global__ __launch_bounds__(kPT) void k_parse_check(uint64_t n_runs, const uint64_t *__restrict__ run_off, const uint32_t *__restrict__ sorted,
                                                      unsigned long long *__restrict__ found)
{
    const uint64_t r = (uint64_t)blockIdx.x * kPT + threadIdx.x;
    if (r >= n_runs) return;
    const uint64_t p = run_off[r];
    if (run_off[r + 1] - p < 2) return;
    atomicMin(found, ((unsigned long long)sorted[p + 1] << 32) | sorted[p]);
}

// *unique += the number of groups with n_kept == 1
__global__ __launch_bounds__(kPT) void k_parse_unique(uint64_t n_groups, const uint32_t *__restrict__ n_kept, unsigned long long *__restrict__ unique)
{
    const uint64_t g = (uint64_t)blockIdx.x * kPT + threadIdx.x;
    unsigned long long s = g < n_groups && n_kept[g] == 1 ? 1ull : 0ull;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(unique, s);
}

// heads[row_idx[g]] = the input index of the first record of group g, for the groups with n_kept > 0 (row_idx: the
// exclusive scan of n_kept > 0)
__global__ __launch_bounds__(kPT) void k_parse_row_heads(uint64_t n_groups, const uint32_t *__restrict__ n_kept,
                                                          const uint64_t *__restrict__ row_idx, const uint64_t *__restrict__ group_off,
                                                          const uint32_t *__restrict__ order, uint32_t *__restrict__ heads)
{
    const uint64_t g = (uint64_t)blockIdx.x * kPT + threadIdx.x;
    if (g < n_groups && n_kept[g]) heads[row_idx[g]] = order[group_off[g]];
}

// *bad = min(*bad, i) over the records i = order[0 .. cnt) whose ref_id (the low half of a record's first word) is not
// below n_txps
__global__ __launch_bounds__(kPT) void k_records_ref_check(uint64_t cnt, const uint32_t *__restrict__ order, const uint64_t *__restrict__ rec_words,
                                                            uint32_t n_txps, unsigned long long *__restrict__ bad)
{
    const uint64_t k = (uint64_t)blockIdx.x * kPT + threadIdx.x;
    if (k >= cnt) return;
    const uint32_t i = order[k];
    if ((uint32_t)rec_words[(uint64_t)i * 5] >= n_txps) atomicMin(bad, (unsigned long long)i);
}
static_assert(offsetof(oem_aln_record, ref_id) == 0 && sizeof(oem_aln_record) == 40, "k_records_ref_check reads ref_id from a record's first word");

template <typename In>
int exclusive_scan(In in, uint64_t *out, uint64_t n)
{
    size_t tb = 0;
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n, nullptr));
    DevBuf<uint8_t> tmp;
    OEM_TRY(dev_alloc(&tmp.p, tb, nullptr));
    OEM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, in, out, (int)n, nullptr));
    OEM_HIP(hipStreamSynchronize(nullptr));
    return OEM_OK;
}

} // namespace

int parse_bad_name(const char *who, bool zero_byte, uint64_t record)
{
    if (zero_byte) return fail(OEM_ERR_ARG, "%s: the name of record %llu contains a 0 byte", who, (unsigned long long)record);
    return fail(OEM_ERR_ARG, "%s: record %llu has an empty name", who, (unsigned long long)record);
}

int parse_not_collated(const char *who, uint64_t group, uint64_t record, uint64_t earlier)
{
    return fail(OEM_ERR_STATE,
                "%s: the input is not name-collated: group %llu (first record %llu) has the name of an earlier group (first record %llu); "
                "OEM_COLLATE_SORT accepts such input",
                who, (unsigned long long)group, (unsigned long long)record, (unsigned long long)earlier);
}

int upload_blob_async(const uint8_t *h_bytes, uint64_t n_bytes, const uint64_t *h_off, uint64_t n, uint64_t extra_bytes, uint64_t extra_off,
                      DevBuf<uint8_t> *d_bytes, DevBuf<uint64_t> *d_off)
{
    OEM_TRY(dev_alloc(&d_bytes->p, n_bytes + kBlobPad + extra_bytes, nullptr));
    OEM_TRY(dev_alloc(&d_off->p, n + 1 + extra_off, nullptr));
    OEM_HIP(hipMemcpyAsync(d_off->p, h_off, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, nullptr));
    if (n_bytes) OEM_HIP(hipMemcpyAsync(d_bytes->p, h_bytes, n_bytes, hipMemcpyHostToDevice, nullptr));
    OEM_HIP(hipMemsetAsync(d_bytes->p + n_bytes, 0, kBlobPad, nullptr));
    return OEM_OK;
}

int upload_flags_async(const uint8_t *h_sec, uint64_t n, DevBuf<uint8_t> *d_sec)
{
    OEM_TRY(dev_alloc(&d_sec->p, n + kFlagPad, nullptr)); // (read through aligned 4-byte words: padded)
    OEM_HIP(hipMemcpyAsync(d_sec->p, h_sec, n, hipMemcpyHostToDevice, nullptr));
    OEM_HIP(hipMemsetAsync(d_sec->p + n, 0, kFlagPad, nullptr));
    return OEM_OK;
}

int records_ref_check(uint64_t m, const uint32_t *d_order, const oem_aln_record *d_in, uint32_t n_txps, uint64_t *bad)
{
    DevBuf<unsigned long long> d_bad;
    unsigned long long b = kNoRecord;
    OEM_TRY(dev_alloc(&d_bad.p, 1, nullptr));
    OEM_HIP(hipMemcpy(d_bad.p, &b, sizeof b, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_records_ref_check, grid_for(m), dim3(kPT), 0, nullptr, m, d_order, (const uint64_t *)d_in, n_txps, d_bad.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpy(&b, d_bad.p, sizeof b, hipMemcpyDeviceToHost));
    *bad = b;
    return OEM_OK;
}

// The names of the records idx[0 .. k) (input indices) gathered from the resident input into one dense, padded blob on
// the device -- the checked groups' heads, the rows' names -- with its k + 1 offsets from 0 and its size.
int gather_input_names(const uint32_t *d_idx, uint64_t k, const uint8_t *d_names, const uint64_t *d_name_off, DevBuf<uint64_t> *d_off_out,
                       DevBuf<uint8_t> *d_blob_out, uint64_t *n_bytes)
{
    OEM_TRY(dev_alloc(&d_off_out->p, k + 1, nullptr));
    OEM_TRY(gather_name_offsets(d_idx, k, d_name_off, d_off_out->p));
    OEM_HIP(hipMemcpy(n_bytes, d_off_out->p + k, sizeof(uint64_t), hipMemcpyDeviceToHost));
    OEM_TRY(dev_alloc(&d_blob_out->p, *n_bytes + 16, nullptr));
    return gather_names(d_idx, k, d_names, d_name_off, d_off_out->p, 0, *n_bytes, d_blob_out->p, nullptr, nullptr);
}


int parse_survivors(const oem_aln_record *d_in, uint64_t n, bool always, DevBuf<uint32_t> *d_order_parse, uint64_t *m)
{
    DevBuf<uint32_t> d_keep;
    DevBuf<uint64_t> d_at;
    OEM_TRY(dev_alloc(&d_keep.p, n + 1, nullptr));
    OEM_TRY(dev_alloc(&d_at.p, n + 1, nullptr));
    hipLaunchKernelGGL(k_parse_keep, grid_for(n + 1), dim3(kPT), 0, nullptr, n, (const uint64_t *)d_in, d_keep.p);
    OEM_HIP(hipGetLastError());
    hipcub::TransformInputIterator<uint64_t, U32ToU64, const uint32_t *> in(d_keep.p, U32ToU64());
    OEM_TRY(exclusive_scan(in, d_at.p, n + 1));
    OEM_HIP(hipMemcpy(m, d_at.p + n, sizeof *m, hipMemcpyDeviceToHost));
    if (*m && (*m < n || always)) {
        OEM_TRY(dev_alloc(&d_order_parse->p, *m, nullptr));
        hipLaunchKernelGGL(k_parse_compact, grid_for(n), dim3(kPT), 0, nullptr, n, (const uint32_t *)d_keep.p, (const uint64_t *)d_at.p,
                           d_order_parse->p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipStreamSynchronize(nullptr));
    }
    return OEM_OK;
}

int parse_survivor_names(const uint8_t *d_names, uint64_t n_bytes, const uint64_t *d_name_off, uint64_t n, const uint32_t *d_order_parse,
                         uint64_t m, const uint8_t *d_sec, DevBuf<uint8_t> *d_dense, DevBuf<uint64_t> *d_dense_off,
                         DevBuf<uint8_t> *d_dense_sec, uint64_t *dense_bytes, uint64_t *bad_record, bool *zero_byte)
{
    DevBuf<unsigned long long> d_bad;
    OEM_TRY(dev_alloc(&d_bad.p, 2, nullptr));
    const unsigned long long bad0[2] = {kNoRecord, kNoRecord};
    unsigned long long bad[2];
    OEM_HIP(hipMemcpy(d_bad.p, bad0, sizeof bad0, hipMemcpyHostToDevice));
    *bad_record = kNoRecord;
    *zero_byte = false;
    *dense_bytes = n_bytes;
    if (!d_order_parse) {
        launch_collate_validate(nullptr, d_names, 0, n_bytes, d_name_off, 0, n, d_bad.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpy(bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
        if (bad[0] != kNoRecord || bad[1] != kNoRecord) {
            *zero_byte = !(bad[1] < bad[0]);
            *bad_record = bad[1] < bad[0] ? bad[1] : bad[0];
        }
        return OEM_OK;
    }
    OEM_TRY(dev_alloc(&d_dense_off->p, m + 1, nullptr));
    OEM_TRY(gather_name_offsets(d_order_parse, m, d_name_off, d_dense_off->p));
    launch_collate_validate(nullptr, d_names, 0, 0, d_dense_off->p, 0, m, d_bad.p); // the empty names, from the offsets alone
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpy(bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
    const uint64_t m_ok = bad[1] != kNoRecord ? bad[1] : m; // the survivors before the first empty name
    OEM_HIP(hipMemcpy(dense_bytes, d_dense_off->p + m_ok, sizeof *dense_bytes, hipMemcpyDeviceToHost));
    OEM_TRY(dev_alloc(&d_dense->p, *dense_bytes + 16, nullptr));
    if (m_ok) {
        const bool flags = d_sec && m_ok == m;
        if (flags) OEM_TRY(dev_alloc(&d_dense_sec->p, ((m + 8) / 8) * 8, nullptr));
        OEM_TRY(gather_names(d_order_parse, m_ok, d_names, d_name_off, d_dense_off->p, 0, *dense_bytes, d_dense->p, flags ? d_sec : nullptr,
                             flags ? d_dense_sec->p : nullptr));
        launch_collate_validate(nullptr, d_dense->p, 0, *dense_bytes, d_dense_off->p, 0, m_ok, d_bad.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpy(bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
    }
    if (bad[0] != kNoRecord || bad[1] != kNoRecord) { // (a 0 byte can only have been found before the first empty name)
        const uint64_t at = bad[0] != kNoRecord ? bad[0] : bad[1];
        uint32_t record = 0;
        OEM_HIP(hipMemcpy(&record, d_order_parse + at, sizeof record, hipMemcpyDeviceToHost));
        *zero_byte = bad[0] != kNoRecord;
        *bad_record = record;
    }
    return OEM_OK;
}

int parse_check_repeat(const char *who, const uint8_t *d_chk, const uint64_t *d_chk_off, uint64_t chk_bytes, uint64_t nchk, uint64_t *found)
{
    *found = ~0ull;
    const uint64_t chk_cell[2] = {0, nchk};
    CollateInput in;
    in.who = who;
    in.cell_rec_off = chk_cell;
    in.mode = kCollateSort;
    in.chunk_bytes = collate_chunk_bytes();
    in.d_names = d_chk;
    in.d_name_off = d_chk_off;
    in.d_n_bytes = chk_bytes;
    CollateResident runs; // order: the checked groups sorted by name, stably; group_off: where a name starts
    double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    OEM_TRY(collate_resident(in, 0, 1, 0, 0, 0, info, &runs));
    if (runs.n_groups == nchk) return OEM_OK;
    DevBuf<unsigned long long> d_found;
    unsigned long long f = ~0ull;
    OEM_TRY(dev_alloc(&d_found.p, 1, nullptr));
    OEM_HIP(hipMemcpy(d_found.p, &f, sizeof f, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_parse_check, grid_for(runs.n_groups), dim3(kPT), 0, nullptr, runs.n_groups, (const uint64_t *)runs.group_off.p,
                       (const uint32_t *)runs.order.p, d_found.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpy(&f, d_found.p, sizeof f, hipMemcpyDeviceToHost));
    *found = f;
    return OEM_OK;
}

int parse_count_unique(uint64_t n_groups, const uint32_t *d_n_kept, uint64_t *unique)
{
    DevBuf<unsigned long long> d_u;
    unsigned long long u = 0;
    OEM_TRY(dev_alloc(&d_u.p, 1, nullptr));
    OEM_HIP(hipMemcpy(d_u.p, &u, sizeof u, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_parse_unique, grid_for(n_groups), dim3(kPT), 0, nullptr, n_groups, d_n_kept, d_u.p);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpy(&u, d_u.p, sizeof u, hipMemcpyDeviceToHost));
    *unique = u;
    return OEM_OK;
}

int parse_row_index(const uint32_t *d_n_kept, uint64_t n, uint64_t *d_row_idx)
{
    hipcub::TransformInputIterator<uint64_t, NonZeroToU64, const uint32_t *> in(d_n_kept, NonZeroToU64());
    return exclusive_scan(in, d_row_idx, n);
}

namespace {

// out[k] = global[order[k]]: the collated order as 64-bit session-global input indices.  order holds resident indices
// below n; an index that is not (there is none) reads nothing and writes kNoRecord.
__global__ __launch_bounds__(kPT) void k_order_global(uint64_t m, uint64_t n, const uint32_t *__restrict__ order,
                                                       const uint64_t *__restrict__ global, uint64_t *__restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * kPT + threadIdx.x;
    if (k >= m) return;
    const uint32_t i = order[k];
    out[k] = i < n ? global[i] : kNoRecord;
}

int tail_bad_ref(const ParseTail &t, uint64_t resident, uint32_t ref_id)
{
    uint64_t at = resident;
    if (t.d_global) OEM_HIP(hipMemcpy(&at, t.d_global + resident, sizeof at, hipMemcpyDeviceToHost));
    return fail(OEM_ERR_ARG, "%s: record %llu: ref_id %u is not below n_txps", t.who, (unsigned long long)at, ref_id);
}

} // namespace

int parse_tail(ParseTail &t)
{
    const char *who = t.who;
    const uint64_t m = t.m;
    const bool sorting = t.mode == kCollateSort, dense = t.dense;
    const uint32_t n_txps = t.n_txps;
    const int model = t.model;
    oem_parse_info &pi = *t.pi;
    double none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double *last = t.last ? t.last : none;
    DevBuf<oem_aln_record> d_sorted;

    // -- collate: the survivors as one cell -----------------------------------------------------------------------------
    const uint64_t one_cell[2] = {0, m};
    CollateResident cr;
    {
        CollateInput in;
        in.who = who;
        in.cell_rec_off = one_cell;
        in.mode = t.mode;
        in.chunk_bytes = collate_chunk_bytes();
        in.d_names = dense ? t.d_dense.p : t.d_names.p;
        in.d_name_off = dense ? t.d_dense_off.p : t.d_name_off.p;
        in.d_n_bytes = t.dense_bytes;
        in.d_secondary = dense ? t.d_dense_sec.p : t.d_sec.p;
        double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        OEM_TRY(collate_resident(in, 0, 1, 0, 0, 0, info, &cr));
    }
    t.d_dense.reset();
    t.d_dense_sec.reset();
    t.d_dense_off.reset();
    t.d_sec.reset();
    if (dense) OEM_TRY(order_compose(m, t.d_order_parse.p, cr.order.p));
    t.d_order_parse.reset();
    const uint64_t ng = cr.n_groups;
    pi.n_groups = ng;

    // -- the collation check --------------------------------------------------------------------------------------------
    if (!sorting && t.sort_check_num) {
        const uint64_t nchk = std::min<uint64_t>(t.sort_check_num, ng);
        pi.n_checked = nchk;
        last[2] = (double)nchk;
        if (nchk > 1) {
            DevBuf<uint32_t> d_heads;
            DevBuf<uint64_t> d_chk_off;
            DevBuf<uint8_t> d_chk;
            uint64_t chk_bytes = 0;
            OEM_TRY(dev_alloc(&d_heads.p, nchk, nullptr));
            hipLaunchKernelGGL(k_parse_heads, grid_for(nchk), dim3(kPT), 0, nullptr, nchk, (const uint64_t *)cr.group_off.p,
                               (const uint32_t *)cr.order.p, d_heads.p);
            OEM_HIP(hipGetLastError());
            OEM_TRY(gather_input_names(d_heads.p, nchk, t.d_names.p, t.d_name_off.p, &d_chk_off, &d_chk, &chk_bytes));
            uint64_t found = ~0ull;
            OEM_TRY(parse_check_repeat(who, d_chk.p, d_chk_off.p, chk_bytes, nchk, &found));
            if (found != ~0ull) {
                const uint64_t g = found >> 32, earlier = found & 0xffffffffull;
                uint32_t rec_g = 0, rec_e = 0;
                OEM_HIP(hipMemcpy(&rec_g, d_heads.p + g, sizeof rec_g, hipMemcpyDeviceToHost));
                OEM_HIP(hipMemcpy(&rec_e, d_heads.p + earlier, sizeof rec_e, hipMemcpyDeviceToHost));
                return parse_not_collated(who, g, rec_g, rec_e);
            }
        }
    }

    if (t.on_groups) t.on_groups(ng);
    if (t.out_order) OEM_HIP(hipMemcpy(t.out_order, cr.order.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    if (t.out_order64 && t.d_global) {
        DevBuf<uint64_t> d_order64;
        OEM_TRY(dev_alloc(&d_order64.p, m, nullptr));
        hipLaunchKernelGGL(k_order_global, grid_for(m), dim3(kPT), 0, nullptr, m, m, (const uint32_t *)cr.order.p, t.d_global, d_order64.p);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpy(t.out_order64, d_order64.p, sizeof(uint64_t) * m, hipMemcpyDeviceToHost));
    }
    if (t.out_group_off) OEM_HIP(hipMemcpy(t.out_group_off, cr.group_off.p, sizeof(uint64_t) * (ng + 1), hipMemcpyDeviceToHost));

    // -- gather and filter ----------------------------------------------------------------------------------------------
    FilterResult r;
    FilterCells fc;
    bool host = t.host_only;
    if (!host) {
        const oem_aln_record *d_recs = t.d_in.p;
        if (sorting || dense) {
            OEM_TRY(dev_alloc(&d_sorted.p, m, nullptr));
            OEM_TRY(records_gather(m, cr.order.p, t.d_in.p, d_sorted.p));
            t.d_in.reset(); // the records are held twice only for the length of the gather
            d_recs = d_sorted.p;
            last[0] = 1;
        }
        fc.n_cells = 1;
        OEM_TRY(filter_device_resident(who, *t.filters, t.txp_len, n_txps, *t.tab, d_recs, (const unsigned long long *)cr.group_off.p, ng,
                                       (const unsigned long long *)cr.cell_group_off.p, model >= 0, &r, &fc));
        if (r.bad_ref_record != kNoRecord) { // a collated position: the caller knows its records by their input index
            uint32_t at = 0;
            OEM_HIP(hipMemcpy(&at, cr.order.p + r.bad_ref_record, sizeof at, hipMemcpyDeviceToHost));
            oem_aln_record rec;
            if (t.h_records) rec = t.h_records[at];
            else OEM_HIP(hipMemcpy(&rec, d_recs + r.bad_ref_record, sizeof rec, hipMemcpyDeviceToHost));
            return tail_bad_ref(t, at, rec.ref_id);
        }
        host = r.host_rerun;
    }

    if (host) { // the host loop: order and group_off come down, the host gathers the records
        last[3] = 1;
        std::vector<uint32_t> order(m), kept(ng);
        std::vector<uint64_t> goff(ng + 1);
        OEM_HIP(hipMemcpy(order.data(), cr.order.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
        OEM_HIP(hipMemcpy(goff.data(), cr.group_off.p, sizeof(uint64_t) * (ng + 1), hipMemcpyDeviceToHost));
        std::vector<oem_aln_record> sorted(m);
        if (t.h_records) {
            for (uint64_t k = 0; k < m; ++k) sorted[k] = t.h_records[order[k]];
        } else { // no host copy of the input: the survivors come down once, collated on the device
            if (!d_sorted.p) {
                OEM_TRY(dev_alloc(&d_sorted.p, m, nullptr));
                OEM_TRY(records_gather(m, cr.order.p, t.d_in.p, d_sorted.p));
            }
            OEM_HIP(hipMemcpy(sorted.data(), d_sorted.p, sizeof(oem_aln_record) * m, hipMemcpyDeviceToHost));
        }
        t.d_in.reset();
        d_sorted.reset();
        cr.order.reset();
        cr.group_off.reset();
        cr.cell_group_off.reset();
        if (t.h_names) {
            t.d_names.reset();
            t.d_name_off.reset();
        }
        for (uint64_t k = 0; k < m; ++k)
            if (sorted[k].ref_id >= n_txps) return tail_bad_ref(t, order[k], sorted[k].ref_id);
        oem_builder hb;
        hb.f = *t.filters;
        hb.txp_len.assign(t.txp_len, t.txp_len + n_txps);
        OEM_TRY(add_groups_host(&hb, sorted.data(), goff.data(), ng, kept.data(), who));
        if (hb.tid.size() >= (1ull << 32)) return fail(OEM_ERR_ARG, "%s: a resident store needs fewer than 2^32 alignments", who);
        pi.n_reads = hb.row_ptr.size() - 1;
        for (uint64_t g = 0; g < ng; ++g)
            if (kept[g] == 1) ++pi.unique_alignments;
        if (t.want_rows && t.h_names) {
            uint64_t row_bytes = 0, row = 0;
            t.out_row_name_off[0] = 0;
            for (uint64_t g = 0; g < ng; ++g) {
                if (!kept[g]) continue;
                const uint32_t i = order[goff[g]];
                std::memcpy(t.out_row_names + row_bytes, t.h_names + t.h_name_off[i], t.h_name_off[i + 1] - t.h_name_off[i]);
                row_bytes += t.h_name_off[i + 1] - t.h_name_off[i];
                t.out_row_name_off[++row] = row_bytes;
            }
        } else if (t.want_rows) { // the rows' heads go up, the resident names are gathered as the device path gathers them
            std::vector<uint32_t> heads;
            for (uint64_t g = 0; g < ng; ++g)
                if (kept[g]) heads.push_back(order[goff[g]]);
            const uint64_t n_rows = heads.size();
            DevBuf<uint32_t> d_heads;
            DevBuf<uint64_t> d_row_off;
            DevBuf<uint8_t> d_rows;
            uint64_t row_bytes = 0;
            if (n_rows) {
                OEM_TRY(dev_alloc(&d_heads.p, n_rows, nullptr));
                OEM_HIP(hipMemcpy(d_heads.p, heads.data(), sizeof(uint32_t) * n_rows, hipMemcpyHostToDevice));
                OEM_TRY(gather_input_names(d_heads.p, n_rows, t.d_names.p, t.d_name_off.p, &d_row_off, &d_rows, &row_bytes));
            }
            if (t.on_rows) t.on_rows(n_rows, row_bytes);
            t.out_row_name_off[0] = 0;
            if (n_rows) OEM_HIP(hipMemcpy(t.out_row_name_off, d_row_off.p, sizeof(uint64_t) * (n_rows + 1), hipMemcpyDeviceToHost));
            if (row_bytes) OEM_HIP(hipMemcpy(t.out_row_names, d_rows.p, row_bytes, hipMemcpyDeviceToHost));
        }
        t.d_names.reset();
        t.d_name_off.reset();
        if (t.out_kept) std::memcpy(t.out_kept, kept.data(), sizeof(uint32_t) * ng);
        if (t.out_discard) *t.out_discard = hb.dt;
        if (model < 0) OEM_TRY(oem_builder_store_create(&hb, nullptr, t.device, t.opts, t.out));
        else OEM_TRY(oem_builder_store_create_coverage(&hb, t.bin_width, model, t.growth_rate, t.device, t.opts, nullptr, t.out));
        return OEM_OK;
    }
    t.d_in.reset();
    d_sorted.reset();

    // -- unique_alignments and the row names, before the store takes the arrays -----------------------------------------
    pi.n_reads = r.n_rows;
    OEM_TRY(parse_count_unique(ng, r.n_kept.p, &pi.unique_alignments));
    if (t.want_rows) {
        DevBuf<uint64_t> d_row_idx, d_row_off;
        DevBuf<uint32_t> d_heads;
        DevBuf<uint8_t> d_rows;
        uint64_t row_bytes = 0;
        if (r.n_rows) {
            OEM_TRY(dev_alloc(&d_row_idx.p, ng + 1, nullptr));
            OEM_TRY(dev_alloc(&d_heads.p, r.n_rows, nullptr));
            OEM_TRY(parse_row_index(r.n_kept.p, ng + 1, d_row_idx.p)); // (n_kept has n_groups + 1 entries, the last one 0)
            hipLaunchKernelGGL(k_parse_row_heads, grid_for(ng), dim3(kPT), 0, nullptr, ng, (const uint32_t *)r.n_kept.p,
                               (const uint64_t *)d_row_idx.p, (const uint64_t *)cr.group_off.p, (const uint32_t *)cr.order.p, d_heads.p);
            OEM_HIP(hipGetLastError());
            d_row_idx.reset();
            OEM_TRY(gather_input_names(d_heads.p, r.n_rows, t.d_names.p, t.d_name_off.p, &d_row_off, &d_rows, &row_bytes));
        }
        if (t.on_rows) t.on_rows(r.n_rows, row_bytes);
        t.out_row_name_off[0] = 0;
        if (r.n_rows) OEM_HIP(hipMemcpy(t.out_row_name_off, d_row_off.p, sizeof(uint64_t) * (r.n_rows + 1), hipMemcpyDeviceToHost));
        if (row_bytes) OEM_HIP(hipMemcpy(t.out_row_names, d_rows.p, row_bytes, hipMemcpyDeviceToHost));
    }
    cr.order.reset();
    cr.group_off.reset();
    cr.cell_group_off.reset();
    t.d_names.reset();
    t.d_name_off.reset();

    return filter_result_to_store(who, r, n_txps, ng, t.bin_width, model, t.growth_rate, t.device, t.opts, t.out_kept, t.out_discard, t.out);
}

void records_names_last_call(double *out8) { std::memcpy(out8, g_records_names_last, sizeof g_records_names_last); }

} // namespace oem

using namespace oem;

extern "C" int oem_store_create_records_names(const oem_filters *filters, const uint64_t *txp_len, uint32_t n_txps,
                                              const oem_aln_record *records, uint64_t n_records, const uint8_t *names,
                                              const uint64_t *name_off, const uint8_t *secondary, uint32_t mode, uint64_t sort_check_num,
                                              uint32_t bin_width, int model, double growth_rate, int device, const oem_store_opts *opts,
                                              uint32_t *out_order, uint64_t *out_group_off, uint32_t *out_kept, uint8_t *out_row_names,
                                              uint64_t *out_row_name_off, oem_discard_table *out_discard, oem_parse_info *out_info,
                                              oem_store **out)
{
    OEM_API_BEGIN
    const char *who = "oem_store_create_records_names";
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    // the checks of oem_store_create_records and of oem_collate_names, before any device use
    OEM_TRY(check_store_from_records(who, filters, txp_len, n_txps, bin_width, model, opts));
    if (!name_off) return fail(OEM_ERR_ARG, "%s: name_off is NULL", who);
    const uint64_t n = n_records, whole[2] = {0, n};
    if (n > kCollateMaxBatch)
        return fail(OEM_ERR_ARG, "%s: %llu records: the names are collated as one batch of at most 2^31 - 2", who, (unsigned long long)n);
    OEM_TRY(check_collate_input(who, names, name_off, n, whole, 1, mode));
    if (n && !records) return fail(OEM_ERR_ARG, "%s: records is NULL", who);
    if ((out_row_names == nullptr) != (out_row_name_off == nullptr))
        return fail(OEM_ERR_ARG, "%s: out_row_names and out_row_name_off must both be NULL or both be given", who);
    std::vector<float> tab;
    const bool host_only = !filter_prob_table(filters->score_prob_denom, tab);
    OEM_TRY(ensure_device(device));

    const bool sorting = mode == kCollateSort, want_rows = out_row_names != nullptr;
    double last[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // [0] k_records_gather ran, [1] the survivors' names were gathered, [2] checked groups, [3] host loop
    std::memset(g_records_names_last, 0, sizeof g_records_names_last);
    oem_parse_info pi;
    std::memset(&pi, 0, sizeof pi);

    // -- upload -------------------------------------------------------------------------------------------------------
    const uint64_t n_bytes = name_off[n];
    DevBuf<oem_aln_record> d_in;
    DevBuf<uint8_t> d_names, d_sec;
    DevBuf<uint64_t> d_name_off;
    DevBuf<uint32_t> d_order_parse;
    uint64_t m = 0;
    if (n) {
        OEM_TRY(dev_alloc(&d_in.p, n, nullptr));
        OEM_TRY(dev_alloc(&d_names.p, n_bytes + 16, nullptr));
        OEM_TRY(dev_alloc(&d_name_off.p, n + 1, nullptr));
        OEM_HIP(hipMemcpy(d_name_off.p, name_off, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice));
        OEM_HIP(hipMemset(d_names.p + n_bytes, 0, 16));
        if (secondary && sorting) { // (read through aligned 4-byte words: padded)
            OEM_TRY(dev_alloc(&d_sec.p, n + 8, nullptr));
            OEM_HIP(hipMemset(d_sec.p + n, 0, 8));
            OEM_HIP(hipMemcpy(d_sec.p, secondary, n, hipMemcpyHostToDevice));
        }
        OEM_HIP(hipStreamSynchronize(nullptr)); // (the lanes do not wait for the null stream)
        OEM_TRY(upload_records(records, n, d_in.p));
        std::vector<uint64_t> byte_cut;
        const uint64_t chunk = collate_chunk_bytes();
        for (uint64_t b = 0; b < n_bytes; b += chunk) byte_cut.push_back(b);
        byte_cut.push_back(n_bytes);
        OEM_TRY(filter_upload_measure<uint8_t>(names, d_names.p, byte_cut.data(), byte_cut.size() - 1, 1, nullptr,
                                               [](hipStream_t, uint64_t, uint64_t) {}));

        // -- the survivors ---------------------------------------------------------------------------------------------
        OEM_TRY(parse_survivors(d_in.p, n, false, &d_order_parse, &m));
    }
    pi.n_parsed = m;
    pi.n_unmapped = n - m;
    const bool dense = m < n; // there are unmapped records: the survivors' names are gathered, the orders composed

    if (m == 0) { // nothing survives: the store of no groups, as oem_store_create_records makes it
        const uint64_t no_groups[1] = {0};
        d_in.reset();
        d_names.reset();
        if (out_group_off) out_group_off[0] = 0;
        if (out_row_name_off) out_row_name_off[0] = 0;
        OEM_TRY(oem_store_create_records(filters, txp_len, n_txps, records, no_groups, 0, bin_width, model, growth_rate, device, opts, nullptr,
                                         out_discard, out));
        if (out_info) *out_info = pi;
        std::memcpy(g_records_names_last, last, sizeof last);
        return OEM_OK;
    }

    // -- the names of the survivors, checked ----------------------------------------------------------------------------
    DevBuf<uint8_t> d_dense, d_dense_sec;
    DevBuf<uint64_t> d_dense_off;
    uint64_t dense_bytes = n_bytes;
    {
        uint64_t bad_record = kNoRecord;
        bool zero_byte = false;
        OEM_TRY(parse_survivor_names(d_names.p, n_bytes, d_name_off.p, n, dense ? d_order_parse.p : nullptr, m, d_sec.p, &d_dense, &d_dense_off,
                                     &d_dense_sec, &dense_bytes, &bad_record, &zero_byte));
        if (bad_record != kNoRecord) return parse_bad_name(who, zero_byte, bad_record);
        if (dense) last[1] = 1;
    }

    // -- the tail: collate, check, gather, filter, store, row names (parse_tail) ------------------------------------------
    ParseTail t;
    t.who = who;
    t.filters = filters;
    t.txp_len = txp_len;
    t.n_txps = n_txps;
    t.tab = &tab;
    t.host_only = host_only;
    t.mode = mode;
    t.sort_check_num = sort_check_num;
    t.bin_width = bin_width;
    t.model = model;
    t.growth_rate = growth_rate;
    t.device = device;
    t.opts = opts;
    t.m = m;
    t.dense = dense;
    t.dense_bytes = dense_bytes;
    std::swap(t.d_in.p, d_in.p);
    std::swap(t.d_names.p, d_names.p);
    std::swap(t.d_sec.p, d_sec.p);
    std::swap(t.d_name_off.p, d_name_off.p);
    std::swap(t.d_order_parse.p, d_order_parse.p);
    std::swap(t.d_dense.p, d_dense.p);
    std::swap(t.d_dense_sec.p, d_dense_sec.p);
    std::swap(t.d_dense_off.p, d_dense_off.p);
    t.h_records = records;
    t.h_names = names;
    t.h_name_off = name_off;
    t.out_order = out_order;
    t.out_group_off = out_group_off;
    t.out_kept = out_kept;
    t.out_row_names = out_row_names;
    t.out_row_name_off = out_row_name_off;
    t.want_rows = want_rows;
    t.out_discard = out_discard;
    t.pi = &pi;
    t.last = last;
    t.out = out;
    OEM_TRY(parse_tail(t));
    if (out_info) *out_info = pi;
    std::memcpy(g_records_names_last, last, sizeof last);
    return OEM_OK;
    OEM_API_END("oem_store_create_records_names")
}
