// oem_testing.hip -- hooks of the TEST-ONLY library (liboarfish_em_testing.so, -DOEM_TESTING).
//
// Nothing in this file is part of the product (liboarfish_em.so is linked without it) or of the
// public header.  tests/ and scripts/ use it to look inside a resident store (layout hashes), to
// hammer the stopping-rule kernel in isolation, to run the remote folds on crafted queues, and --
// together with the OEM_TESTING build of oem_comm.cpp -- to run the row-sharded loop with several
// shards on one GPU.
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "oem_barcode_correct.h"
#include "oem_cells.h"
#include "oem_cells_barcodes_stream.h"
#include "oem_collate.h"
#include "oem_collate_device.h"
#include "oem_gene_counts.h"
#include "oem_shortest_f64.h"

using namespace oem;

// Test hook (not in the public header): 64-bit hashes of the resident tiled layout, so that the
// device-built layout can be checked element for element against the host-built one.
// out[0..3] = n_tiles, n_rows, n_local, n_remote; out[4..13] = tiles, perm, codes, w, r_tid, r_w,
// r_row, r_slot, q_dst, bucket_base; out[14] (if asked for) = 1 when the device built it; returns OEM_ERR_STATE when the store has no tiled layout.
extern "C" int oem_debug_layout_hash(oem_store *s, uint64_t *out, uint32_t n_out)
{
    OEM_API_BEGIN
    if (!s || !out || n_out < 14) return fail(OEM_ERR_ARG, "oem_debug_layout_hash: bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    OEM_HIP(hipSetDevice(s->device));
    const DeviceTiled &t = s->tiled;
    if (!t.present) return fail(OEM_ERR_STATE, "oem_debug_layout_hash: no tiled layout");
    auto hash_dev = [&](const void *d, size_t bytes, uint64_t *h) -> int {
        std::vector<uint64_t> buf((bytes + 7) / 8, 0);
        if (bytes) OEM_HIP(hipMemcpy(buf.data(), d, bytes, hipMemcpyDeviceToHost));
        uint64_t x = 0x9e3779b97f4a7c15ull ^ bytes;
        for (uint64_t v : buf) { x ^= v; x *= 0xff51afd7ed558ccdull; x ^= x >> 29; }
        *h = x;
        return OEM_OK;
    };
    // array lengths follow from the descriptors: slices and remote records end with the last tile
    uint64_t w_slots = 0, c_slots = 0;
    if (t.n_tiles) {
        TileDesc last;
        OEM_HIP(hipMemcpy(&last, t.tiles + (t.n_tiles - 1), sizeof(last), hipMemcpyDeviceToHost));
        w_slots = last.w_base; c_slots = last.c_base;
        for (uint32_t i = 0; i < kTileSlices; ++i) { w_slots += last.width[i]; c_slots += (last.width[i] + 1u) / 2; }
    }
    out[0] = t.n_tiles; out[1] = t.n_rows; out[2] = t.n_local; out[3] = t.n_remote;
    const size_t wsz = s->csr.w_is_f64 ? 8 : 4;
    OEM_TRY(hash_dev(t.tiles, sizeof(TileDesc) * t.n_tiles, &out[4]));
    OEM_TRY(hash_dev(t.perm, 4 * t.n_rows, &out[5]));
    OEM_TRY(hash_dev(t.codes, 4 * (c_slots + 1) * 64, &out[6]));
    OEM_TRY(hash_dev(s->csr.w_is_f64 ? (const void *)t.w64 : (const void *)t.w32, wsz * (w_slots + 1) * 64, &out[7]));
    if (!t.r_tid || !t.r_row || !t.r_slot)
        return fail(OEM_ERR_STATE, "oem_debug_layout_hash: the builders' remote streams were dropped (set OEM_KEEP_UNPACKED=1)");
    OEM_TRY(hash_dev(t.r_tid, 4 * t.n_remote, &out[8]));
    OEM_TRY(hash_dev(s->csr.w_is_f64 ? (const void *)t.r_w64 : (const void *)t.r_w32, wsz * t.n_remote, &out[9]));
    OEM_TRY(hash_dev(t.r_row, 2 * t.n_remote, &out[10]));
    OEM_TRY(hash_dev(t.r_slot, 4 * t.n_remote, &out[11]));
    OEM_TRY(hash_dev(t.q_dst, 2 * t.n_remote, &out[12]));
    OEM_TRY(hash_dev(t.bucket_base, 4 * ((size_t)t.n_buckets + 1), &out[13]));
    if (n_out > 14) out[14] = t.built_on_device ? 1 : 0;
    if (n_out > 17) { // the slim form the kernels read (oem_layout_pack.hip)
        OEM_TRY(hash_dev(t.sd, 4 * (size_t)t.n_sd, &out[15]));
        out[16] = 0;
        if (t.packed) OEM_TRY(hash_dev(t.r_pk, 4 * t.n_remote, &out[16]));
        out[17] = t.packed ? 1 : 0;
    }
    return OEM_OK;
    OEM_API_END("oem_debug_layout_hash")
}


// Test hook: what oem::knob() returns in THIS library (the environment variable in the test-only build; the
// product's knob() is compiled without getenv and returns its default, checked on the object file).
extern "C" long oem_debug_knob(const char *name, long dflt) { return oem::knob(name, dflt); }

// Test hook: the groups of this thread's last per-cell call (oem_em_run_cells, oem_em_run_cells_sparse,
// oem_em_run_cells_coverage_sparse) and the path each one took.  *n_groups = the number of groups; out[3 g .. 3 g + 2]
// = c0, c1, 1 when group g ran batched / 0 when cell by cell, for the first `cap` groups.
extern "C" int oem_debug_cells_last_paths(uint32_t *n_groups, uint32_t *out, uint32_t cap)
{
    if (!n_groups || (cap && !out)) return fail(OEM_ERR_ARG, "oem_debug_cells_last_paths: bad argument");
    const std::vector<CellsGroupPath> &p = cells_last_paths();
    *n_groups = (uint32_t)p.size();
    for (size_t g = 0; g < p.size() && g < cap; ++g) {
        out[3 * g] = p[g].c0;
        out[3 * g + 1] = p[g].c1;
        out[3 * g + 2] = p[g].batched;
    }
    return OEM_OK;
}

// Test hook: which instantiations the launchers last launched (LaunchRecord, oem_internal.h) -- on store `s` since the
// previous call of this hook on it (the record is cleared: a step that launches nothing of a family reads as none), or,
// with s == NULL, in the last batched group of this thread's last per-cell call, whose stores the caller never sees.
// out[0..6]   k_em_tile:     launched, wide window, f64 weights, coding (0 plain, 1 bytes, 2 fused, 3 words), packed
//                            records, non-temporal streams, per-cell batch
// out[7..11]  k_em_tile_e:   launched, f64 weights, fused, packed records, non-temporal streams
// out[12..14] k_remote_fold: launched, non-temporal queue (kNTQ), workgroups per bucket
extern "C" int oem_debug_last_launch(oem_store *s, uint32_t *out, uint32_t n_out)
{
    if (!out || n_out < 15) return fail(OEM_ERR_ARG, "oem_debug_last_launch: bad argument");
    LaunchRecord r;
    if (s) {
        std::lock_guard<std::mutex> lk(s->mu);
        r = s->last_launch;
        s->last_launch = LaunchRecord();
    } else {
        for (const CellsGroupPath &p : cells_last_paths())
            if (p.batched) r = p.launch;
    }
    const uint32_t v[15] = {r.tile & 1u, (r.tile >> 1) & 1u, (r.tile >> 2) & 1u, (r.tile >> 3) & 3u, (r.tile >> 5) & 1u,
                            (r.tile >> 6) & 1u, (r.tile >> 7) & 1u,
                            r.batch & 1u, (r.batch >> 1) & 1u, (r.batch >> 2) & 1u, (r.batch >> 3) & 1u, (r.batch >> 4) & 1u,
                            r.fold & 1u, (r.fold >> 1) & 1u, r.fold >> 8};
    std::memcpy(out, v, sizeof(v));
    return OEM_OK;
}

// out[0..2] = kernel ms of this thread's last oem_assignment_text under OEM_TEXT_TIMING=1: measure, scan, emit (all chunks)
extern "C" int oem_debug_text_last_timing(float *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_text_last_timing: NULL argument");
    text_last_timing(out);
    return OEM_OK;
}

// out[0..2] = kernel ms of this thread's last oem_count_matrix_text under OEM_MTX_TIMING=1: measure, scan, emit (all chunks)
extern "C" int oem_debug_mtx_last_timing(float *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_mtx_last_timing: NULL argument");
    mtx_last_timing(out);
    return OEM_OK;
}

// out[0..5] = this thread's last oem_quant_text / oem_ambig_text: chunks, workgroup tiles that went through the LDS stage,
// tiles written directly, then kernel ms under OEM_QUANT_TIMING=1: measure, scan, emit (all chunks)
extern "C" int oem_debug_quant_last_call(double *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_quant_last_call: NULL argument");
    quant_last_call(out);
    return OEM_OK;
}

// out[0..7] = this thread's last oem_collate_names: key rounds (the most of any batch), upload chunks, batches; under
// OEM_COLLATE_TIMING=1 ms of the name uploads, of the kernels behind each chunk, of the rounds and the cut after the upload
// (HIP events) and of the copies into pinned staging (host clock); the rounds that had to sort
extern "C" int oem_debug_collate_last_call(double *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_collate_last_call: NULL argument");
    collate_last_call(out);
    return OEM_OK;
}

// Test hook: the host walk of oem_collate.h -- std::sort of each cell's record indices with the rule's comparator, then
// the cut -- with oem_collate_names' arguments (checked by the caller) and outputs; n_threads workers take the cells one
// by one, the way the reference's workers do.  An empty name or a 0 byte is OEM_ERR_ARG naming the record.
extern "C" int oem_test_collate_host(const uint8_t *names, const uint64_t *name_off, const uint8_t *secondary, uint64_t n_records,
                                     const uint64_t *cell_rec_off, uint32_t n_cells, uint32_t mode, uint32_t n_threads,
                                     uint32_t *out_order, uint64_t *out_group_off, uint64_t *out_n_groups, uint64_t *out_cell_group_off)
{
    OEM_API_BEGIN
    if (!name_off || !cell_rec_off || !out_order || !out_group_off || !out_n_groups || !out_cell_group_off || (n_records && !names))
        return fail(OEM_ERR_ARG, "oem_test_collate_host: NULL argument");
    bool zero_byte = false;
    const uint64_t bad = collate_first_bad_name(names, name_off, n_records, &zero_byte);
    if (bad != kCollateNoRecord)
        return fail(OEM_ERR_ARG, zero_byte ? "oem_test_collate_host: the name of record %llu contains a 0 byte"
                                           : "oem_test_collate_host: record %llu has an empty name", (unsigned long long)bad);
    std::atomic<uint32_t> next{0};
    auto work = [&]() {
        for (uint32_t c = next.fetch_add(1); c < n_cells; c = next.fetch_add(1))
            collate_host_cell(names, name_off, secondary, cell_rec_off[c], cell_rec_off[c + 1], mode, out_order);
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads && t < n_cells; ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    collate_host_cut(names, name_off, n_records, cell_rec_off, n_cells, out_order, out_group_off, out_n_groups, out_cell_group_off);
    return OEM_OK;
    OEM_API_END("oem_test_collate_host")
}

// out[0..7] = this thread's last oem_collate_barcodes (or the barcode stage of the one call), and the stages of its last
// oem_em_run_cells_records_barcodes_sparse: the layouts of oem_collate_device.h
extern "C" int oem_debug_collate_barcodes_last_call(double *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_collate_barcodes_last_call: NULL argument");
    collate_barcodes_last_call(out);
    return OEM_OK;
}
extern "C" int oem_debug_cells_barcodes_last_call(double *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_cells_barcodes_last_call: NULL argument");
    cells_barcodes_last_call(out);
    return OEM_OK;
}
// Test hook: the barcode table of the last any-order barcoded session that reached finish in this library (8 words):
// [0] rebuilds, [1] the longest probe in slots, [2] 1 when a probe went past the table's end, [3] the most doublings one
// rebuild covered (above 1: several inside one batch), [4] the final capacity, [5] labels, [6] misses.
extern "C" int oem_debug_barcode_table_last(uint64_t *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_barcode_table_last: NULL argument");
    barcode_table_last(out);
    return OEM_OK;
}

// Test hook: the host walk of oem_collate.h's barcode rule (collate_barcodes_host) with oem_collate_barcodes' arguments
// (checked by the caller) and outputs.  An empty barcode or a 0 byte is OEM_ERR_ARG naming the first such record.
extern "C" int oem_test_collate_barcodes_host(const uint8_t *barcodes, const uint64_t *barcode_off, uint64_t n_records, uint32_t *out_order,
                                              uint64_t *out_cell_rec_off, uint64_t *out_n_cells)
{
    OEM_API_BEGIN
    if (!barcode_off || !out_order || !out_cell_rec_off || !out_n_cells || (n_records && !barcodes))
        return fail(OEM_ERR_ARG, "oem_test_collate_barcodes_host: NULL argument");
    bool zero_byte = false;
    const uint64_t bad = collate_barcodes_host(barcodes, barcode_off, n_records, out_order, out_cell_rec_off, out_n_cells, &zero_byte);
    if (bad != kCollateNoRecord)
        return fail(OEM_ERR_ARG, zero_byte ? "oem_test_collate_barcodes_host: the barcode of record %llu contains a 0 byte"
                                           : "oem_test_collate_barcodes_host: record %llu has an empty barcode", (unsigned long long)bad);
    return OEM_OK;
    OEM_API_END("oem_test_collate_barcodes_host")
}

// Test hook: the host walk of oem_collate.h's UMI rule (dedup_umis_host) with oem_dedup_umis' arguments and outputs.  The
// offsets are taken as checked; an order entry that is not below n_records and a UMI with a 0 byte are OEM_ERR_ARG, worded
// as the device call words them.
extern "C" int oem_test_dedup_umis_host(const uint8_t *umis, const uint64_t *umi_off, const uint32_t *flags, uint64_t n_records,
                                        const uint32_t *order, uint64_t n_positions, const uint64_t *group_off, uint64_t n_groups,
                                        const uint64_t *cell_group_off, uint32_t n_cells, uint8_t *out_dup, uint64_t *out_survivor,
                                        uint64_t *out_cell_dups)
{
    OEM_API_BEGIN
    if (!umi_off || !group_off || !cell_group_off || !out_dup || !out_survivor || !out_cell_dups || (n_positions && !order) ||
        (umi_off[n_records] && !umis))
        return fail(OEM_ERR_ARG, "oem_test_dedup_umis_host: NULL argument");
    for (uint64_t k = 0; k < n_positions; ++k)
        if (order[k] >= n_records)
            return fail(OEM_ERR_ARG, "oem_test_dedup_umis_host: order[%llu] = %u is not below n_records = %llu", (unsigned long long)k, order[k],
                        (unsigned long long)n_records);
    const uint64_t bad = dedup_first_bad_umi(umis, umi_off, n_records);
    if (bad != kCollateNoRecord)
        return fail(OEM_ERR_ARG, "oem_test_dedup_umis_host: the UMI of record %llu contains a 0 byte", (unsigned long long)bad);
    dedup_umis_host(umis, umi_off, flags, order, group_off, n_groups, cell_group_off, n_cells, out_dup, out_survivor, out_cell_dups);
    return OEM_OK;
    OEM_API_END("oem_test_dedup_umis_host")
}

// Test hook: the host walk of oem_collate.h's UMI rule (dedup_umis_rule_host) with oem_dedup_umis_rule's arguments and
// outputs.  Checked and worded as the device call: the rule's own argument errors, an order entry that is not below
// n_records, a UMI with a 0 byte, the head of a read that takes part whose ref_id is not below n_txps.
extern "C" int oem_test_dedup_umis_rule_host(const oem_umi_rule *rule, const uint8_t *umis, const uint64_t *umi_off, const uint32_t *flags,
                                             const uint32_t *ref_id, uint64_t n_records, const uint32_t *order, uint64_t n_positions,
                                             const uint64_t *group_off, uint64_t n_groups, const uint64_t *cell_group_off, uint32_t n_cells,
                                             uint8_t *out_dup, uint64_t *out_survivor, uint64_t *out_cell_dups, uint64_t *out_cell_corrected)
{
    OEM_API_BEGIN
    const char *who = "oem_test_dedup_umis_rule_host";
    if (!umi_off || !group_off || !cell_group_off || !out_dup || !out_survivor || !out_cell_dups || (n_positions && !order) ||
        (umi_off[n_records] && !umis))
        return fail(OEM_ERR_ARG, "%s: NULL argument", who);
    const uint32_t *gene_of = rule ? rule->gene_of : nullptr;
    if (rule) {
        if (rule->correct > 1) return fail(OEM_ERR_ARG, "%s: rule->correct = %u is neither 0 nor 1", who, rule->correct);
        if (gene_of && !rule->n_txps) return fail(OEM_ERR_ARG, "%s: rule->gene_of is given and rule->n_txps is 0", who);
        if (gene_of && !ref_id) return fail(OEM_ERR_ARG, "%s: rule->gene_of is given and ref_id is NULL", who);
    }
    for (uint64_t k = 0; k < n_positions; ++k)
        if (order[k] >= n_records)
            return fail(OEM_ERR_ARG, "%s: order[%llu] = %u is not below n_records = %llu", who, (unsigned long long)k, order[k],
                        (unsigned long long)n_records);
    uint64_t bad = dedup_first_bad_umi(umis, umi_off, n_records);
    if (bad != kCollateNoRecord) return fail(OEM_ERR_ARG, "%s: the UMI of record %llu contains a 0 byte", who, (unsigned long long)bad);
    bad = dedup_umis_rule_host(umis, umi_off, flags, ref_id, gene_of, rule ? rule->n_txps : 0u, rule ? rule->correct : 0u, order, group_off,
                               n_groups, cell_group_off, n_cells, out_dup, out_survivor, out_cell_dups, out_cell_corrected);
    if (bad != kCollateNoRecord)
        return fail(OEM_ERR_ARG, "%s: record %llu: ref_id %u is not below n_txps = %u (the head of a read that takes part in the UMI rule)", who,
                    (unsigned long long)bad, ref_id[bad], rule->n_txps);
    return OEM_OK;
    OEM_API_END("oem_test_dedup_umis_rule_host")
}

// Test hook: the host walk of oem_barcode_correct.h (correct_barcodes_host) with oem_correct_barcodes' arguments minus the
// device, checked and worded as the device call.  The table's knobs (OEM_BARCODE_HASH_BITS, OEM_BARCODE_TABLE_SLOTS0) hold
// for the walk's table too.
extern "C" int oem_test_correct_barcodes_host(const oem_barcode_rule *rule, const uint8_t *barcodes, const uint64_t *barcode_off,
                                              uint64_t n_records, uint32_t *out_id, uint8_t *out_status, uint32_t *out_order,
                                              uint64_t *out_cell_rec_off, uint64_t *out_n_cells, uint64_t *out_n_accepted, uint64_t *out_counts)
{
    OEM_API_BEGIN
    const char *who = "oem_test_correct_barcodes_host";
    if (!barcode_off || !out_n_cells || !out_n_accepted) return fail(OEM_ERR_ARG, "%s: barcode_off, out_n_cells or out_n_accepted is NULL", who);
    *out_n_cells = 0;
    *out_n_accepted = 0;
    OEM_TRY(check_barcode_rule(who, rule));
    OEM_TRY(check_barcode_input(who, barcodes, barcode_off, n_records));
    static const uint8_t acgt[4] = {'A', 'C', 'G', 'T'};
    const uint32_t hash_bits = (uint32_t)std::min<long>(std::max<long>(knob("OEM_BARCODE_HASH_BITS", 64), 0), 64);
    const uint64_t slots0 = (uint64_t)std::max<long>(knob("OEM_BARCODE_TABLE_SLOTS0", (long)kBarcodeTableSlots0), 2);
    const BarcodeCorrectHost info =
        correct_barcodes_host(rule->labels, rule->label_off, rule->n_labels, rule->multi, rule->alphabet ? rule->alphabet : acgt,
                              rule->alphabet ? rule->n_alphabet : 4u, barcodes, barcode_off, n_records, out_id, out_status, out_order,
                              out_cell_rec_off, out_n_cells, out_n_accepted, out_counts, hash_bits, slots0);
    if (info.zero_label != kBarcodeNoIndex)
        return fail(OEM_ERR_ARG, "%s: label %llu of the whitelist contains a 0 byte", who, (unsigned long long)info.zero_label);
    if (info.broken) return fail(OEM_ERR_STATE, "%s: the whitelist table is broken", who);
    if (info.equal_j != kBarcodeNoIndex)
        return fail(OEM_ERR_ARG, "%s: labels %llu and %llu of the whitelist are equal", who, (unsigned long long)info.equal_i,
                    (unsigned long long)info.equal_j);
    if (info.zero_barcode != kBarcodeNoIndex)
        return fail(OEM_ERR_ARG, "%s: the barcode of record %llu contains a 0 byte", who, (unsigned long long)info.zero_barcode);
    if (out_cell_rec_off && *out_n_cells == 0) out_cell_rec_off[0] = 0;
    return OEM_OK;
    OEM_API_END("oem_test_correct_barcodes_host")
}

// Test hook: the streamed walk of oem_barcode_correct.h (correct_barcodes_stream_host, "The rule in a session"): the input
// of the hook above cut into n_batches batches at batch_off (n_batches + 1 entries from 0 to the number of records), with
// a flag per record for the unmapped ones (or NULL).  Checked and worded as the hook above.  out_order is 64 bits wide;
// out_cell_label / out_cell_corrected have room for rule->n_labels cells; out_info: the records rejected and deferred.
extern "C" int oem_test_correct_barcodes_stream_host(const oem_barcode_rule *rule, const uint8_t *barcodes, const uint64_t *barcode_off,
                                                     const uint64_t *batch_off, uint64_t n_batches, const uint8_t *unmapped, uint32_t *out_id,
                                                     uint8_t *out_status, uint64_t *out_order, uint64_t *out_cell_rec_off,
                                                     uint32_t *out_cell_label, uint64_t *out_cell_corrected, uint64_t *out_n_cells,
                                                     uint64_t *out_n_accepted, uint64_t *out_counts, uint64_t *out_info)
{
    OEM_API_BEGIN
    const char *who = "oem_test_correct_barcodes_stream_host";
    if (!barcode_off || !batch_off || !out_n_cells || !out_n_accepted || !out_info)
        return fail(OEM_ERR_ARG, "%s: barcode_off, batch_off, out_n_cells, out_n_accepted or out_info is NULL", who);
    *out_n_cells = 0;
    *out_n_accepted = 0;
    OEM_TRY(check_barcode_rule(who, rule));
    OEM_TRY(check_offsets(who, "batch_off", batch_off, n_batches, "batch"));
    const uint64_t n_records = batch_off[n_batches];
    OEM_TRY(check_barcode_input(who, barcodes, barcode_off, n_records));
    static const uint8_t acgt[4] = {'A', 'C', 'G', 'T'};
    const uint32_t hash_bits = (uint32_t)std::min<long>(std::max<long>(knob("OEM_BARCODE_HASH_BITS", 64), 0), 64);
    const uint64_t slots0 = (uint64_t)std::max<long>(knob("OEM_BARCODE_TABLE_SLOTS0", (long)kBarcodeTableSlots0), 2);
    const BarcodeCorrectHost info = correct_barcodes_stream_host(
        rule->labels, rule->label_off, rule->n_labels, rule->multi, rule->alphabet ? rule->alphabet : acgt, rule->alphabet ? rule->n_alphabet : 4u,
        barcodes, barcode_off, batch_off, n_batches, unmapped, out_id, out_status, out_order, out_cell_rec_off, out_cell_label, out_cell_corrected,
        out_n_cells, out_n_accepted, out_counts, out_info, out_info + 1, hash_bits, slots0);
    if (info.zero_label != kBarcodeNoIndex)
        return fail(OEM_ERR_ARG, "%s: label %llu of the whitelist contains a 0 byte", who, (unsigned long long)info.zero_label);
    if (info.broken) return fail(OEM_ERR_STATE, "%s: the whitelist table is broken", who);
    if (info.equal_j != kBarcodeNoIndex)
        return fail(OEM_ERR_ARG, "%s: labels %llu and %llu of the whitelist are equal", who, (unsigned long long)info.equal_i,
                    (unsigned long long)info.equal_j);
    if (info.zero_barcode != kBarcodeNoIndex)
        return fail(OEM_ERR_ARG, "%s: the barcode of record %llu contains a 0 byte", who, (unsigned long long)info.zero_barcode);
    if (out_cell_rec_off && *out_n_cells == 0) out_cell_rec_off[0] = 0;
    return OEM_OK;
    OEM_API_END("oem_test_correct_barcodes_stream_host")
}

// Test hook: the host walk of oem_gene_counts.h (gene_counts_host) with oem_cells_gene_counts' arguments minus the device,
// checked and worded as the device call, and its kind of result.
extern "C" int oem_test_cells_gene_counts_host(const uint64_t *cell_off, uint32_t n_cells, const uint32_t *col, const float *val,
                                               const uint32_t *gene_of, uint32_t n_txps, uint32_t n_genes, oem_cells_result **out)
{
    OEM_API_BEGIN
    const char *who = "oem_test_cells_gene_counts_host";
    if (out) *out = nullptr;
    if (!out) return fail(OEM_ERR_ARG, "%s: out is NULL", who);
    OEM_TRY(gene_counts_check(who, cell_off, n_cells, col, val, gene_of, n_txps, n_genes));
    std::vector<SparseBlock> blocks(1);
    gene_counts_host(cell_off, n_cells, col, val, gene_of, &blocks[0].counts, &blocks[0].col, &blocks[0].val);
    return gene_counts_result(who, n_cells, blocks, out);
    OEM_API_END("oem_test_cells_gene_counts_host")
}

// out[0..5] = this thread's last oem_cells_gene_counts (oem_driver.h, gene_counts_last_call)
extern "C" int oem_debug_gene_counts_last_call(double *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_gene_counts_last_call: NULL argument");
    gene_counts_last_call(out);
    return OEM_OK;
}

// out[0..7] = what the corrections of the last oem_dedup_umis_rule / oem_em_run_cells_records_umis_rule_sparse found
// (oem_collate_device.h, dedup_rule_last_call)
extern "C" int oem_debug_dedup_rule_last_call(double *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_dedup_rule_last_call: NULL argument");
    dedup_rule_last_call(out);
    return OEM_OK;
}

// out[0..7] = this thread's last oem_store_create_records_names: [0] 1 if k_records_gather ran, [1] 1 if the survivors'
// names were gathered, [2] the groups the collation check looked at, [3] 1 if the host loop took the groups
namespace oem { void records_names_last_call(double *out8); }
extern "C" int oem_debug_records_names_last_call(double *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_records_names_last_call: NULL argument");
    records_names_last_call(out);
    return OEM_OK;
}

// Test hook: the host walk of oem_collate.h's bulk rule (parse_bulk_host) with oem_store_create_records_names' input
// arguments (checked by the caller).  out_order (capacity n_records), out_group_off (capacity n_records + 1), out_info:
// n_unmapped, n_parsed, n_groups, n_checked, then the repeat's group, record and earlier record when the collation
// check fails (OEM_ERR_STATE).  A bad name is OEM_ERR_ARG naming the record.
extern "C" int oem_test_parse_bulk_host(const oem_aln_record *records, uint64_t n_records, const uint8_t *names, const uint64_t *name_off,
                                        const uint8_t *secondary, uint32_t mode, uint64_t sort_check_num, uint32_t *out_order,
                                        uint64_t *out_group_off, uint64_t *out_info)
{
    OEM_API_BEGIN
    if (!name_off || !out_order || !out_group_off || !out_info || (n_records && (!names || !records)))
        return fail(OEM_ERR_ARG, "oem_test_parse_bulk_host: NULL argument");
    const ParseBulk pb = parse_bulk_host(records, n_records, names, name_off, secondary, mode, sort_check_num, out_order, out_group_off);
    const uint64_t info[7] = {pb.n_unmapped, pb.n_parsed, pb.n_groups, pb.n_checked, pb.repeat_group, pb.repeat_record, pb.earlier_record};
    std::memcpy(out_info, info, sizeof info);
    if (pb.bad_record != kCollateNoRecord)
        return fail(OEM_ERR_ARG, pb.zero_byte ? "oem_test_parse_bulk_host: the name of record %llu contains a 0 byte"
                                              : "oem_test_parse_bulk_host: record %llu has an empty name", (unsigned long long)pb.bad_record);
    if (pb.repeat_group != kCollateNoRecord)
        return fail(OEM_ERR_STATE, "oem_test_parse_bulk_host: group %llu (first record %llu) has the name of an earlier group (first record %llu)",
                    (unsigned long long)pb.repeat_group, (unsigned long long)pb.repeat_record, (unsigned long long)pb.earlier_record);
    return OEM_OK;
    OEM_API_END("oem_test_parse_bulk_host")
}

// Test hook: the host build of oem_shortest_f64.h.  The texts of the n finite f64 with these bits, one after the other
// in `text`; off[i] .. off[i + 1] are the bytes of value i (off has n + 1 entries, from the length function; the
// emitter must end where it says).  OEM_ERR_ARG for a value that is not finite or a text that would pass `cap`.
extern "C" int oem_test_shortest_f64(const uint64_t *bits, uint64_t n, uint8_t *text, uint64_t cap, uint64_t *off)
{
    if ((n && !bits) || !off || (cap && !text)) return fail(OEM_ERR_ARG, "oem_test_shortest_f64: NULL argument");
    off[0] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!f64_is_finite(bits[i])) return fail(OEM_ERR_ARG, "oem_test_shortest_f64: value %llu is not finite", (unsigned long long)i);
        off[i + 1] = off[i] + shortest_f64_len(bits[i]);
        if (off[i + 1] > cap) return fail(OEM_ERR_ARG, "oem_test_shortest_f64: text holds %llu bytes", (unsigned long long)cap);
        if (emit_shortest_f64(text + off[i], bits[i]) != text + off[i + 1])
            return fail(OEM_ERR_STATE, "oem_test_shortest_f64: value %llu: the emitter and the length function differ", (unsigned long long)i);
    }
    return OEM_OK;
}

// out[0..1] = kernel ms of this thread's last oem_assignment_text_lz4 under OEM_TEXT_TIMING=1: k_lz4_blocks, scan +
// k_lz4_gather (all chunks); its measure / scan / emit are in oem_debug_text_last_timing
extern "C" int oem_debug_text_lz4_last_timing(float *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_text_lz4_last_timing: NULL argument");
    text_lz4_last_timing(out);
    return OEM_OK;
}

// out[0..5] = this thread's last device batch call (oem_builder_add_groups_device, oem_store_create_records) under
// OEM_FILTER_TIMING=1: from HIP events, ms of the record uploads, k_filter_measure (both summed over the chunks), the two
// scans, k_filter_emit, and the fraction of the measure kernels' time during which a record copy was in flight; from the
// host clock, ms of the copies into pinned staging.  All zero when the host loop took the batch without a device pass.
extern "C" int oem_debug_filter_last_timing(float *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_filter_last_timing: NULL argument");
    filter_last_timing(out);
    return OEM_OK;
}

// out[0..4] = this thread's last projected device batch call (oem_builder_add_projected_groups_device,
// oem_store_create_projected_records): ms of k_proj_measure (summed over the chunks) and of k_proj_emit from HIP events
// under OEM_FILTER_TIMING=1, ms of finishing the unsure alignments on the host (host clock), the number of alignments the
// host finished with libm's expf and the number emitted.  All zero when the host loop took the batch without a device pass.
extern "C" int oem_debug_proj_last_pass(double *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_proj_last_pass: NULL argument");
    proj_last_pass(out);
    return OEM_OK;
}

// Test hook: the filtered CSR of the last group of cells that went through the device pass of the records path
// (oem_em_run_cells_records_sparse, a records session) while OEM_TEST_KEEP_RECORDS_CSR=1 was set: dims3 = reads,
// alignments, cells; row_ptr (reads + 1, u32), tid / as_prob as bits / start / end (alignments each), cell_row_off
// (cells + 1).  Any output may be NULL: call once for the sizes, once for the arrays.
extern "C" int oem_debug_cells_records_last_csr(uint64_t *dims3, uint32_t *row_ptr, uint32_t *tid, uint32_t *as_prob_bits,
                                                uint32_t *start, uint32_t *end, uint64_t *cell_row_off)
{
    return cells_records_last_csr(dims3, row_ptr, tid, as_prob_bits, start, end, cell_row_off);
}

// Test hook: ends a records session (oem_records_stream_*) as oem_records_stream_finish does, but copies the joined CSR
// to the host instead of making a store of it, so that the join can be compared bit for bit.  dims3 = rows, alignments,
// groups, always; row_ptr (rows + 1, u32), tid / as_prob as bits / start / end / strand (alignments each; the last three
// are left alone by a session without a model) and kept (groups) are copied when they fit caps3 (OEM_ERR_ARG otherwise);
// any of them may be NULL.  *join_ms (or NULL): k_stream_concat by HIP events.
namespace oem {
int records_stream_finish_csr(oem_records_stream *s, uint64_t *dims3, const uint64_t *caps3, uint32_t *row_ptr, uint32_t *tid,
                              uint32_t *as_prob_bits, uint32_t *start, uint32_t *end, uint8_t *strand, uint32_t *kept,
                              oem_discard_table *dt, float *join_ms);
float records_stream_last_join_ms();
}
extern "C" int oem_debug_records_stream_finish_csr(oem_records_stream *s, uint64_t *dims3, const uint64_t *caps3, uint32_t *row_ptr,
                                                   uint32_t *tid, uint32_t *as_prob_bits, uint32_t *start, uint32_t *end,
                                                   uint8_t *strand, uint32_t *kept, oem_discard_table *dt, float *join_ms)
{
    OEM_API_BEGIN
    return records_stream_finish_csr(s, dims3, caps3, row_ptr, tid, as_prob_bits, start, end, strand, kept, dt, join_ms);
    OEM_API_END("oem_debug_records_stream_finish_csr")
}

// ms of k_stream_concat (HIP events) in this thread's last oem_records_stream_finish; 0 when there was nothing to join
extern "C" int oem_debug_records_stream_last_join(float *out)
{
    if (!out) return fail(OEM_ERR_ARG, "oem_debug_records_stream_last_join: NULL argument");
    *out = records_stream_last_join_ms();
    return OEM_OK;
}

// Test hook: the n caller bytes at `data` as one LZ4 frame, by the path oem_assignment_text_lz4 compresses a chunk with
// (upload, k_lz4_blocks, scan, k_lz4_gather; blocks of OEM_LZ4_BLOCK_BYTES), so that tests can feed crafted inputs.
// *out_len = the frame's length, always; the frame is copied to out when it fits cap (else OEM_ERR_ARG).
extern "C" int oem_test_lz4_frame(const uint8_t *data, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len)
{
    OEM_API_BEGIN
    if ((!data && n) || (!out && cap) || !out_len) return fail(OEM_ERR_ARG, "oem_test_lz4_frame: bad argument");
    *out_len = 0;
    OEM_TRY(ensure_device(0));
    hipStream_t st = nullptr;
    OEM_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    std::unique_ptr<uint8_t[]> frame;
    uint64_t len = 0, n_blocks = 0, raw_blocks = 0;
    const int rc = lz4_frame_from_host(data, n, st, &frame, &len, &n_blocks, &raw_blocks);
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    OEM_TRY(rc);
    *out_len = len;
    if (len > cap) return fail(OEM_ERR_ARG, "oem_test_lz4_frame: the frame has %llu bytes, out holds %llu", (unsigned long long)len, (unsigned long long)cap);
    std::memcpy(out, frame.get(), len);
    return OEM_OK;
    OEM_API_END("oem_test_lz4_frame")
}

// ---------------------------------------------------------------------------
// Stress test of k_reldiff_swap_clear's last-block election (oem_kernels.hip): the stopping
// decision of every EM run (em.rs:194-218) is taken by the workgroup that draws the last ticket,
// from a running maximum the other workgroups published with device-scope atomics just before
// taking theirs.  Each launch gets a fresh (prev, curr) pair whose rel-diff maximum is known
// exactly -- one planted element at a pseudo-random position, (curr - prev) / prev =
// 0.75 + launch * 2^-20, every other element strictly below 0.5 -- and the decision workgroup's
// view of it (EmState::last_rel) is recorded after every launch.  out_last_rel[i] must equal the
// planted value bit for bit; a stale or partial maximum shows up as a smaller number.
// ---------------------------------------------------------------------------
namespace {

__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}

__global__ __launch_bounds__(256) void k_stress_case(double *__restrict__ prev, double *__restrict__ curr, uint32_t n,
                                                     uint32_t launch, uint32_t seed)
{
    const uint32_t pos = mix32(seed ^ (launch * 0x9e3779b9u)) % n;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        prev[i] = 1.0;
        const double below = (double)(mix32(i * 2654435761u + launch) & 0xffffu) * (0.5 / 65536.0);
        curr[i] = i == pos ? 1.75 + (double)launch * (1.0 / 1048576.0) : 1.0 + below;
    }
}

__global__ void k_stress_record(const EmState *state, double *out, uint32_t launch) { out[launch] = state->last_rel; }

} // namespace

extern "C" int oem_test_reldiff_stress(uint32_t n_txps, uint32_t n_launches, uint32_t seed, int device,
                                       double *out_last_rel /* n_launches */)
{
    OEM_API_BEGIN
    if (!n_txps || !n_launches || !out_last_rel) return fail(OEM_ERR_ARG, "oem_test_reldiff_stress: bad argument");
    OEM_HIP(hipSetDevice(device));
    oem_store s; // only the stream is used by the launcher
    s.device = device;
    OEM_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    double *prev = nullptr, *curr = nullptr, *rec = nullptr;
    EmState *st = nullptr;
    int rc = OEM_OK;
    do {
        if (hipMalloc((void **)&prev, sizeof(double) * n_txps) != hipSuccess ||
            hipMalloc((void **)&curr, sizeof(double) * n_txps) != hipSuccess ||
            hipMalloc((void **)&rec, sizeof(double) * n_launches) != hipSuccess ||
            hipMalloc((void **)&st, sizeof(EmState)) != hipSuccess ||
            hipMemsetAsync(st, 0, sizeof(EmState), s.stream) != hipSuccess) {
            rc = fail(OEM_ERR_OOM, "oem_test_reldiff_stress: device allocation failed");
            break;
        }
        EmParams p{n_txps, 0xffffffffu, 0xffffffffu, -1.0}; // never stops: rel_diff >= 0 is never < -1
        uint32_t g = (n_txps + 255) / 256;
        if (g > 1024) g = 1024;
        for (uint32_t i = 0; i < n_launches && rc == OEM_OK; ++i) {
            hipLaunchKernelGGL(k_stress_case, dim3(g), dim3(256), 0, s.stream, prev, curr, n_txps, i, seed);
            rc = launch_reldiff_swap_clear(&s, prev, curr, st, p);
            hipLaunchKernelGGL(k_stress_record, dim3(1), dim3(1), 0, s.stream, st, rec, i);
        }
        if (rc != OEM_OK) break;
        if (hipMemcpyAsync(out_last_rel, rec, sizeof(double) * n_launches, hipMemcpyDeviceToHost, s.stream) != hipSuccess ||
            hipStreamSynchronize(s.stream) != hipSuccess)
            rc = fail(OEM_ERR_HIP, "oem_test_reldiff_stress: read-back failed");
    } while (false);
    hipFree(prev); hipFree(curr); hipFree(rec); hipFree(st);
    hipStreamDestroy(s.stream);
    s.stream = nullptr;
    return rc;
    OEM_API_END("oem_test_reldiff_stress")
}

// ---------------------------------------------------------------------------
// The remote folds on crafted queues (tests/test_remote_fold_gpu.py).  A fold is a scatter-add: with integer-valued
// doubles every order of summation gives the same bits, so each of the hooks below can be held to numpy's add.at
// exactly.  oem_test_lane_runs runs the lane-level helpers of oem_lane_runs.h alone, one wavefront per case; the three
// others launch one fold kernel once on caller-made arrays (launchers: oem_internal.h) and copy the results back.
// Every index a kernel would use unchecked is checked here first.
// ---------------------------------------------------------------------------
#include "oem_lane_runs.h"

namespace {

// Lanes < n_active of every wavefront call keys_repeat and sum_runs_of_equal_keys, the others stay out under a real
// branch (a partial exec mask, as in the last trip of a fold's loop); vals / out_vals: [lane][kStride].
template <int kStride>
__global__ __launch_bounds__(256) void k_test_lane_runs(const uint32_t *__restrict__ keys, const double *__restrict__ vals, uint32_t n_waves,
                                                        uint32_t n_active, double *__restrict__ out_vals, uint32_t *__restrict__ out_repeat)
{
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (wave >= n_waves) return;
    const size_t i = (size_t)wave * 64 + lane;
    const uint32_t d = keys[i];
    double v[kStride];
#pragma unroll
    for (int j = 0; j < kStride; ++j) v[j] = vals[i * kStride + j];
    if (lane < n_active) {
        const bool rep = keys_repeat<kStride>(d);
        sum_runs_of_equal_keys<kStride, kStride>(d, v);
        if (lane == 0) out_repeat[wave] = rep ? 1u : 0u;
    }
#pragma unroll
    for (int j = 0; j < kStride; ++j) out_vals[i * kStride + j] = v[j];
}

// device copies of a hook's arrays: freed when the hook returns, whichever way
struct TestArrays {
    std::vector<void *> mem;
    ~TestArrays() { for (void *p : mem) (void)hipFree(p); }
    template <typename T>
    int up(T **d, const T *h, size_t n, hipStream_t st) // (one element at least: an empty queue still has an address)
    {
        void *p = nullptr;
        OEM_HIP(hipMalloc(&p, sizeof(T) * (n ? n : 1)));
        mem.push_back(p);
        *d = static_cast<T *>(p);
        if (n && h) OEM_HIP(hipMemcpyAsync(p, h, sizeof(T) * n, hipMemcpyHostToDevice, st));
        else OEM_HIP(hipMemsetAsync(p, 0, sizeof(T) * (n ? n : 1), st));
        return OEM_OK;
    }
};
struct TestStream {
    hipStream_t st = nullptr;
    ~TestStream() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } }
};

// what every fold reads unchecked: bucket b's range [bucket_base[b], bucket_base[b + 1]) of the queue, destinations inside
// the LDS window; the buckets cover the transcripts
int check_fold_queue(const char *who, const uint32_t *bucket_base, uint32_t n_buckets, const uint16_t *q_dst, uint32_t n_txps)
{
    if (!bucket_base || !n_txps || n_buckets != (n_txps + kBucket - 1) / kBucket)
        return fail(OEM_ERR_ARG, "%s: n_buckets = %u does not cover n_txps = %u", who, n_buckets, n_txps);
    OEM_TRY(check_offsets(who, "bucket_base", bucket_base, n_buckets, "bucket"));
    if (bucket_base[n_buckets] && !q_dst) return fail(OEM_ERR_ARG, "%s: q_dst is NULL", who);
    for (uint32_t i = 0; i < bucket_base[n_buckets]; ++i)
        if (q_dst[i] >= kBucket) return fail(OEM_ERR_ARG, "%s: q_dst[%u] = %u is outside the window", who, i, (unsigned)q_dst[i]);
    return OEM_OK;
}

} // namespace

// keys [n_waves][64], vals and out_vals [n_waves][64][stride], out_repeat [n_waves]: the wave's keys_repeat<stride>
extern "C" int oem_test_lane_runs(uint32_t stride, const uint32_t *keys, const double *vals, uint32_t n_waves, uint32_t n_active,
                                  double *out_vals, uint32_t *out_repeat, int device)
{
    OEM_API_BEGIN
    if ((stride != 1 && stride != 2) || !keys || !vals || !n_waves || !n_active || n_active > 64 || !out_vals || !out_repeat)
        return fail(OEM_ERR_ARG, "oem_test_lane_runs: bad argument");
    OEM_HIP(hipSetDevice(device));
    TestStream ts;
    OEM_HIP(hipStreamCreateWithFlags(&ts.st, hipStreamNonBlocking));
    TestArrays a;
    const size_t n = (size_t)n_waves * 64;
    uint32_t *d_keys = nullptr, *d_rep = nullptr;
    double *d_vals = nullptr, *d_out = nullptr;
    OEM_TRY(a.up(&d_keys, keys, n, ts.st));
    OEM_TRY(a.up(&d_vals, vals, n * stride, ts.st));
    OEM_TRY(a.up(&d_out, (const double *)nullptr, n * stride, ts.st));
    OEM_TRY(a.up(&d_rep, (const uint32_t *)nullptr, n_waves, ts.st));
    const uint32_t grid = (n_waves + 3) / 4;
    if (stride == 1) hipLaunchKernelGGL(k_test_lane_runs<1>, dim3(grid), dim3(256), 0, ts.st, d_keys, d_vals, n_waves, n_active, d_out, d_rep);
    else hipLaunchKernelGGL(k_test_lane_runs<2>, dim3(grid), dim3(256), 0, ts.st, d_keys, d_vals, n_waves, n_active, d_out, d_rep);
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipMemcpyAsync(out_vals, d_out, sizeof(double) * n * stride, hipMemcpyDeviceToHost, ts.st));
    OEM_HIP(hipMemcpyAsync(out_repeat, d_rep, sizeof(uint32_t) * n_waves, hipMemcpyDeviceToHost, ts.st));
    OEM_HIP(hipStreamSynchronize(ts.st));
    return OEM_OK;
    OEM_API_END("oem_test_lane_runs")
}

// One launch of k_remote_fold<ntq, threads> with n_groups workgroups per bucket: cnt (n_txps, in and out) += the queue's
// entries, entry i of bucket b into cnt[b * kBucket + q_dst[i]].  done: -1 no loop state, else EmState::done of the launch.
extern "C" int oem_test_remote_fold(const uint32_t *bucket_base, uint32_t n_buckets, const double *queue, const uint16_t *q_dst,
                                    double *cnt, uint32_t n_txps, uint32_t n_groups, uint32_t ntq, uint32_t threads, int done, int device)
{
    OEM_API_BEGIN
    const char *who = "oem_test_remote_fold";
    OEM_TRY(check_fold_queue(who, bucket_base, n_buckets, q_dst, n_txps));
    const uint32_t n = bucket_base[n_buckets];
    if (!cnt || (n && !queue) || !n_groups || (threads != 1024 && threads != 256) || done < -1 || done > 1)
        return fail(OEM_ERR_ARG, "%s: bad argument", who);
    EmState h_state;
    std::memset(&h_state, 0, sizeof h_state);
    h_state.done = done > 0 ? 1u : 0u;
    OEM_HIP(hipSetDevice(device));
    TestStream ts;
    OEM_HIP(hipStreamCreateWithFlags(&ts.st, hipStreamNonBlocking));
    TestArrays a;
    uint32_t *d_base = nullptr;
    double *d_queue = nullptr, *d_cnt = nullptr;
    uint16_t *d_dst = nullptr;
    EmState *d_state = nullptr;
    OEM_TRY(a.up(&d_base, bucket_base, (size_t)n_buckets + 1, ts.st));
    OEM_TRY(a.up(&d_queue, queue, n, ts.st));
    OEM_TRY(a.up(&d_dst, q_dst, n, ts.st));
    OEM_TRY(a.up(&d_cnt, (const double *)cnt, n_txps, ts.st));
    if (done >= 0) OEM_TRY(a.up(&d_state, (const EmState *)&h_state, 1, ts.st));
    OEM_TRY(launch_test_remote_fold(ts.st, n_buckets, d_base, d_queue, d_dst, d_cnt, d_state, n_groups, n_txps, ntq != 0, threads));
    OEM_HIP(hipMemcpyAsync(cnt, d_cnt, sizeof(double) * n_txps, hipMemcpyDeviceToHost, ts.st));
    OEM_HIP(hipStreamSynchronize(ts.st));
    return OEM_OK;
    OEM_API_END("oem_test_remote_fold")
}

// One launch of k_remote_fold_b: queue [entry][n_slots], theta and cnt (in and out) [n_txps][n_slots], phases [n_slots]
// (kPhaseRunning 0, kPhaseFinal 1, kPhaseFinished 2).  n_slots must be the library's kBatch.
extern "C" int oem_test_remote_fold_b(const uint32_t *bucket_base, uint32_t n_buckets, const double *queue, const uint16_t *q_dst,
                                      const double *theta, double *cnt, uint32_t n_txps, uint32_t n_groups, const uint32_t *phases,
                                      uint32_t n_slots, int device)
{
    OEM_API_BEGIN
    const char *who = "oem_test_remote_fold_b";
    if (n_slots != (uint32_t)kBatch) return fail(OEM_ERR_ARG, "%s: n_slots = %u, the library is built for %d", who, n_slots, kBatch);
    OEM_TRY(check_fold_queue(who, bucket_base, n_buckets, q_dst, n_txps));
    const uint32_t n = bucket_base[n_buckets];
    if (!theta || !cnt || !phases || (n && !queue) || !n_groups) return fail(OEM_ERR_ARG, "%s: bad argument", who);
    BatchState h_state[kBatch];
    std::memset(h_state, 0, sizeof h_state);
    for (int b = 0; b < kBatch; ++b) {
        if (phases[b] > kPhaseFinished) return fail(OEM_ERR_ARG, "%s: phases[%d] = %u", who, b, phases[b]);
        h_state[b].phase = phases[b];
    }
    OEM_HIP(hipSetDevice(device));
    TestStream ts;
    OEM_HIP(hipStreamCreateWithFlags(&ts.st, hipStreamNonBlocking));
    TestArrays a;
    uint32_t *d_base = nullptr;
    double *d_queue = nullptr, *d_theta = nullptr, *d_cnt = nullptr;
    uint16_t *d_dst = nullptr;
    BatchState *d_state = nullptr;
    OEM_TRY(a.up(&d_base, bucket_base, (size_t)n_buckets + 1, ts.st));
    OEM_TRY(a.up(&d_queue, queue, (size_t)n * kBatch, ts.st));
    OEM_TRY(a.up(&d_dst, q_dst, n, ts.st));
    OEM_TRY(a.up(&d_theta, theta, (size_t)n_txps * kBatch, ts.st));
    OEM_TRY(a.up(&d_cnt, (const double *)cnt, (size_t)n_txps * kBatch, ts.st));
    OEM_TRY(a.up(&d_state, (const BatchState *)h_state, (size_t)kBatch, ts.st));
    OEM_TRY(launch_test_remote_fold_b(ts.st, n_buckets, d_base, d_queue, d_dst, d_theta, d_cnt, d_state, n_groups, n_txps));
    OEM_HIP(hipMemcpyAsync(cnt, d_cnt, sizeof(double) * n_txps * kBatch, hipMemcpyDeviceToHost, ts.st));
    OEM_HIP(hipStreamSynchronize(ts.st));
    return OEM_OK;
    OEM_API_END("oem_test_remote_fold_b")
}

// One launch of k_multi_fold_reldiff over every bucket: cell p owns transcripts [p T, (p + 1) T) of n_txps = n_cells T;
// phases [n_cells]; theta, cnt, out (n_txps each) and rel_bits (n_cells: BatchState::rel_bits) go in and come back.
extern "C" int oem_test_multi_fold_reldiff(const uint32_t *bucket_base, uint32_t n_buckets, const double *queue, const uint16_t *q_dst,
                                           double *theta, double *cnt, double *out, uint32_t n_txps, uint32_t T, const uint32_t *phases,
                                           uint64_t *rel_bits, int device)
{
    OEM_API_BEGIN
    const char *who = "oem_test_multi_fold_reldiff";
    OEM_TRY(check_fold_queue(who, bucket_base, n_buckets, q_dst, n_txps));
    const uint32_t n = bucket_base[n_buckets];
    if (!theta || !cnt || !out || !phases || !rel_bits || (n && !queue) || !T || n_txps % T)
        return fail(OEM_ERR_ARG, "%s: bad argument", who);
    const uint32_t n_cells = n_txps / T;
    std::vector<BatchState> h_state(n_cells);
    std::memset(h_state.data(), 0, sizeof(BatchState) * n_cells);
    for (uint32_t p = 0; p < n_cells; ++p) {
        if (phases[p] > kPhaseFinished) return fail(OEM_ERR_ARG, "%s: phases[%u] = %u", who, p, phases[p]);
        h_state[p].phase = phases[p];
        h_state[p].rel_bits = rel_bits[p];
    }
    OEM_HIP(hipSetDevice(device));
    TestStream ts;
    OEM_HIP(hipStreamCreateWithFlags(&ts.st, hipStreamNonBlocking));
    TestArrays a;
    uint32_t *d_base = nullptr;
    double *d_queue = nullptr, *d_theta = nullptr, *d_cnt = nullptr, *d_out = nullptr;
    uint16_t *d_dst = nullptr;
    BatchState *d_state = nullptr;
    OEM_TRY(a.up(&d_base, bucket_base, (size_t)n_buckets + 1, ts.st));
    OEM_TRY(a.up(&d_queue, queue, n, ts.st));
    OEM_TRY(a.up(&d_dst, q_dst, n, ts.st));
    OEM_TRY(a.up(&d_theta, (const double *)theta, n_txps, ts.st));
    OEM_TRY(a.up(&d_cnt, (const double *)cnt, n_txps, ts.st));
    OEM_TRY(a.up(&d_out, (const double *)out, n_txps, ts.st));
    OEM_TRY(a.up(&d_state, (const BatchState *)h_state.data(), n_cells, ts.st));
    OEM_TRY(launch_test_multi_fold_reldiff(ts.st, n_buckets, d_base, d_queue, d_dst, d_theta, d_cnt, d_out, d_state, n_txps, T));
    OEM_HIP(hipMemcpyAsync(theta, d_theta, sizeof(double) * n_txps, hipMemcpyDeviceToHost, ts.st));
    OEM_HIP(hipMemcpyAsync(cnt, d_cnt, sizeof(double) * n_txps, hipMemcpyDeviceToHost, ts.st));
    OEM_HIP(hipMemcpyAsync(out, d_out, sizeof(double) * n_txps, hipMemcpyDeviceToHost, ts.st));
    OEM_HIP(hipMemcpyAsync(h_state.data(), d_state, sizeof(BatchState) * n_cells, hipMemcpyDeviceToHost, ts.st));
    OEM_HIP(hipStreamSynchronize(ts.st));
    for (uint32_t p = 0; p < n_cells; ++p) rel_bits[p] = h_state[p].rel_bits;
    return OEM_OK;
    OEM_API_END("oem_test_multi_fold_reldiff")
}
