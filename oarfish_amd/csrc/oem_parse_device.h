// oem_parse_device.h -- the steps of the bulk parser on the device (oem_records_names.hip) that the one call
// (oem_store_create_records_names) and the names sessions (oem_records_stream_push_names and _push_sort,
// oem_records_stream.hip) share.  Everything runs on the null stream and leaves it idle.  Also the host memory of the
// staging queue (oem_stage_queue.h) for the sessions that parse on the device: these and the barcoded cells sessions.
#pragma once

#include <functional>
#include <vector>

#include "oem_collate_device.h"
#include "oem_filter_device.h"
#include "oem_stage_queue.h"

namespace oem {

// A staged batch's host memory: page-locked on `device` so that the worker uploads straight from it, else pageable.
// False when neither is to be had.
inline bool stage_host_alloc(int device, size_t bytes, StageMem *m)
{
    if (hipSetDevice(device) == hipSuccess && hipHostMalloc(&m->p, bytes, hipHostMallocPortable) == hipSuccess) {
        m->pinned = true;
        return true;
    }
    (void)hipGetLastError();
    m->pinned = false;
    m->p = malloc(bytes);
    return m->p != nullptr;
}
inline void stage_host_free(StageMem &m)
{
    if (m.pinned) (void)hipHostFree(m.p);
    else free(m.p);
    m = StageMem();
}

// A staged blob up: d_bytes (n_bytes + 16 + extra_bytes allocated, the 16 bytes behind n_bytes zero) and d_off (n + 1 +
// extra_off allocated, the n + 1 offsets copied); the flags form: n flags with 8 zero bytes behind them.  The copies
// are queued on the null stream from memory that stays until the caller has synchronized.
int upload_blob_async(const uint8_t *h_bytes, uint64_t n_bytes, const uint64_t *h_off, uint64_t n, uint64_t extra_bytes, uint64_t extra_off,
                      DevBuf<uint8_t> *d_bytes, DevBuf<uint64_t> *d_off);
int upload_flags_async(const uint8_t *h_sec, uint64_t n, DevBuf<uint8_t> *d_sec);

// *bad = the smallest i = d_order[k], k < m, whose record d_in[i] has a ref_id that is not below n_txps, or kNoRecord: a
// batch's survivors are checked where the batch still knows its indices
int records_ref_check(uint64_t m, const uint32_t *d_order, const oem_aln_record *d_in, uint32_t n_txps, uint64_t *bad);

// The survivors of d_in[0 .. n) (the records without OEM_REC_UNMAPPED): *m of them, and order_parse, their input
// indices in ascending order.  order_parse is left empty when it would be the identity (m == n) unless `always`.
int parse_survivors(const oem_aln_record *d_in, uint64_t n, bool always, DevBuf<uint32_t> *d_order_parse, uint64_t *m);

// The names of the m survivors, checked.  d_order_parse NULL: every record survives, the blob is checked where it is.
// Otherwise the survivors' names (and flags, d_sec / d_dense_sec, or NULL) are gathered into d_dense / d_dense_off
// first, so that a skipped record's name is never examined.  *bad_record: kNoRecord, or the input index of the first
// survivor with an empty name or (*zero_byte) a 0 byte in its name; the dense arrays are then unspecified.
int parse_survivor_names(const uint8_t *d_names, uint64_t n_bytes, const uint64_t *d_name_off, uint64_t n, const uint32_t *d_order_parse,
                         uint64_t m, const uint8_t *d_sec, DevBuf<uint8_t> *d_dense, DevBuf<uint64_t> *d_dense_off,
                         DevBuf<uint8_t> *d_dense_sec, uint64_t *dense_bytes, uint64_t *bad_record, bool *zero_byte);

// The collation check over nchk > 1 head names (a dense padded blob with its nchk + 1 offsets): *found = ~0 when no
// name repeats, else (g << 32 | earlier): the smallest group g whose name an earlier group has, and that group.
int parse_check_repeat(const char *who, const uint8_t *d_chk, const uint64_t *d_chk_off, uint64_t chk_bytes, uint64_t nchk, uint64_t *found);

// the number of groups with n_kept == 1
int parse_count_unique(uint64_t n_groups, const uint32_t *d_n_kept, uint64_t *unique);

// The names of the records idx[0 .. k) (indices into d_name_off) gathered into one dense, padded blob on the device
// with its k + 1 offsets from 0 and its size.
int gather_input_names(const uint32_t *d_idx, uint64_t k, const uint8_t *d_names, const uint64_t *d_name_off, DevBuf<uint64_t> *d_off_out,
                       DevBuf<uint8_t> *d_blob_out, uint64_t *n_bytes);

// the exclusive scan of (n_kept > 0) over n entries: a group's row
int parse_row_index(const uint32_t *d_n_kept, uint64_t n, uint64_t *d_row_idx);

// The tail of the bulk parser, from "collate: the survivors as one cell" on (oem_records_names.hip): collate_resident,
// the collation check, records_gather, filter_device_resident, the coverage model, the store and the row-name gather.
// oem_store_create_records_names runs it on its uploaded input, the sorting names session's finish
// (oem_records_stream_push_sort) on its arena.  The resident input: n records of which m > 0 survive, their names as
// a blob (8-byte aligned, padded by 16) with n + 1 offsets, all indexed by the record's RESIDENT index.  The buffers
// are the tail's to release as it goes.
struct ParseTail {
    const char *who = nullptr;
    const oem_filters *filters = nullptr;
    const uint64_t *txp_len = nullptr;
    uint32_t n_txps = 0;
    const std::vector<float> *tab = nullptr; // filter_prob_table of score_prob_denom
    bool host_only = false;                  // ... or there is none
    uint32_t mode = kCollateSort;
    uint64_t sort_check_num = 0;
    uint32_t bin_width = 0;
    int model = -1;
    double growth_rate = 0;
    int device = 0;
    const oem_store_opts *opts = nullptr;

    uint64_t m = 0;
    DevBuf<oem_aln_record> d_in;
    DevBuf<uint8_t> d_names, d_sec; // d_sec: the resident records' flags (padded by 8), or empty
    DevBuf<uint64_t> d_name_off;
    // with unmapped records among the resident ones (`dense`): the survivors' resident indices, ascending, and their
    // names and flags gathered (parse_survivor_names); otherwise the resident arrays are the survivors'
    bool dense = false;
    DevBuf<uint32_t> d_order_parse;
    DevBuf<uint8_t> d_dense, d_dense_sec;
    DevBuf<uint64_t> d_dense_off;
    uint64_t dense_bytes = 0;
    // The caller's input on the host, by resident index (the one call), for the host loop and the ref_id message.  NULL
    // (the session): the host loop brings the survivors down from the device.
    const oem_aln_record *h_records = nullptr;
    const uint8_t *h_names = nullptr;
    const uint64_t *h_name_off = nullptr;
    // NULL: a record's resident index is its input index.  Otherwise (the session) d_global[i] is the 64-bit
    // session-global input index of resident record i; out_order64 and the messages go through it.
    const uint64_t *d_global = nullptr;

    // Outputs, each or NULL.  on_groups(n_groups) is called once the groups are cut and before anything is written,
    // on_rows(n_rows, row_bytes) before the row names are: a caller that cannot size its arrays beforehand sets the
    // pointers there.
    uint32_t *out_order = nullptr;   // m input indices (d_global == NULL)
    uint64_t *out_order64 = nullptr; // m session-global indices (d_global != NULL)
    uint64_t *out_group_off = nullptr;
    uint32_t *out_kept = nullptr;
    uint8_t *out_row_names = nullptr;
    uint64_t *out_row_name_off = nullptr;
    bool want_rows = false;
    std::function<void(uint64_t)> on_groups;
    std::function<void(uint64_t, uint64_t)> on_rows;
    oem_discard_table *out_discard = nullptr;
    oem_parse_info *pi = nullptr; // n_unmapped and n_parsed are the caller's; the tail fills the rest
    double *last = nullptr;       // records_names_last_call's slots [0], [2] and [3], or NULL
    oem_store **out = nullptr;
};
int parse_tail(ParseTail &t);

int parse_bad_name(const char *who, bool zero_byte, uint64_t record);
int parse_not_collated(const char *who, uint64_t group, uint64_t record, uint64_t earlier);

} // namespace oem
