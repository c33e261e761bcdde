// oem_parse_device.h -- the steps of the bulk parser on the device (oem_records_names.hip) that the one call
// (oem_store_create_records_names) and the names session (oem_records_stream_push_names, oem_records_stream.hip) share.
// Everything runs on the null stream and leaves it idle.
#pragma once

#include "oem_collate_device.h"
#include "oem_filter_device.h"

namespace oem {

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

int parse_bad_name(const char *who, bool zero_byte, uint64_t record);
int parse_not_collated(const char *who, uint64_t group, uint64_t record, uint64_t earlier);

} // namespace oem
