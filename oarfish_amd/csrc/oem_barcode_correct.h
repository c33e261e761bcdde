// oem_barcode_correct.h -- raw cell barcodes matched against a whitelist, with one-mismatch correction: the rule of
// oem_correct_barcodes and oem_em_run_cells_records_whitelist_sparse as pure host / device code, and its host walk.
// The host walk is the specification; the device (oem_barcode_correct.hip) is held to it exactly.
//
// The reference wants every record to carry a CORRECTED cell barcode (docs/index.md:308-312); a raw CR tag with one
// sequencing error would be a cell of its own.  Inputs: the n_records raw barcodes (blob + offsets, the empty string
// where the tag is missing), a whitelist of W >= 1 distinct labels (the chemistry's permit list), an alphabet (default
// ACGT) and multi in {0, 1}.
//
//   exact       a record whose barcode is byte-identical to label w: id = w, kBarcodeExact
//   counts      n(w) = the records of the call that are exact for w, whatever their flags; a corrected record never adds
//   neighbours  of a non-empty barcode b that is not exact: the labels of b's length that differ from b in exactly one
//               byte position AND whose byte there is in the alphabet.  b's own byte there may be anything (an N); two Ns
//               have no neighbour; a label byte outside the alphabet is only ever matched exactly
//   choice      none: kBarcodeNoNeighbour.  multi = 0 (STARsolo's 1MM): exactly one neighbour is kBarcodeCorrected to it,
//               more are kBarcodeAmbiguous.  multi = 1: one neighbour is kBarcodeCorrected to it whatever its n; of
//               several the one whose n(w) is STRICTLY largest wins, a tie for the largest is kBarcodeAmbiguous
//   missing     an empty barcode: kBarcodeMissing (no error here)
//   rejected    kBarcodeNoNeighbour, kBarcodeAmbiguous, kBarcodeMissing: id = kBarcodeNoId, the record is in no cell
//   cells       a cell is the accepted records of one label; cells are numbered by their first accepted record in input
//               order and the records keep input order inside a cell (oem_collate_barcodes' numbering: input that holds
//               only whitelisted barcodes gives that call's order / cell_rec_off).  A cell's label is the whitelist's.
//
// A neighbour is found by PROBING, never by comparing all labels: for every byte position and every alphabet byte other
// than the barcode's own, the candidate (the barcode with that one byte replaced) is looked up in the table of
// oem_barcode_table.h.  A label differs from b in exactly one position p and is found only by the candidate of p with
// its own byte, so no neighbour is counted twice.  The hash of oem_barcode_table.h chains over 8-byte words, so the
// candidates of one position share the prefix up to that position's word (barcode_hash_prefix) and cost only the words
// from there on (barcode_hash_from).  The result never depends on the hash, on probe order or on the arrival order of
// atomics: the counts are integer sums, the choice is a function of the set of neighbours and their counts.
//
// THE RULE IN A SESSION (oem_cells_stream_set_whitelist on the any-order barcoded session; the walk is
// correct_barcodes_stream_host).  The input arrives as batches, in ticket order, and n(w) grows with them.
//
//   unmapped    a record with OEM_REC_UNMAPPED takes no part: its barcode is never examined and it adds nothing to n(w).
//               The other records are the survivors S, as in every session.  THE ONE CALL DIFFERS on input that holds
//               unmapped records: its n(w) counts them.  The session equals the one call on the S-arrays.
//   a survivor  may have an empty barcode (kBarcodeMissing); a 0 byte in it is the batch's error
//   per batch   the exact pass gives the exact survivors their label and adds to the session's n(w), which is never reset.
//               The neighbour pass runs over the batch's misses with the counts as they stand.  `found`, the number of
//               neighbours, does not depend on the counts: found == 0 is kBarcodeNoNeighbour, found == 1 is
//               kBarcodeCorrected, and under multi == 0 found >= 2 is kBarcodeAmbiguous -- all final in the batch.  Only
//               multi == 1 with found >= 2 waits for the complete counts: the record is DEFERRED (kBarcodeDeferred, a
//               status that never leaves the library).
//   dropped     a record rejected in its batch (missing, a length no label has, no neighbour, ambiguous under multi == 0)
//               is dropped there: its name, UMI and ref_id are never looked at, and it never enters the arena
//   retained    the accepted and the deferred records: the survivors of everything that follows.  The name and UMI checks
//               and the batch's ref_id check run over them only; the arena keeps them with a 4-byte whitelist id
//               (kBarcodeNoId for a deferred record, kBarcodeCorrectedBit set for a corrected one); a deferred record's
//               barcode and its arena position go to the pending list
//   finish      the neighbour pass once more, over the pending list and with n(w) complete: the winners get their label,
//               the rest is kBarcodeAmbiguous, leaves the arena in the layout by cell and is never gathered
//   cells       numbered by their first accepted record in session order, session order inside a cell.  A cell's first
//               accepted record may be one that was deferred, so the numbering is done at finish from the ids -- a stable
//               sort over the bits the whitelist needs, the runs ranked by their first record, as the one call ends --
//               and never per batch by first sight.  A cell's label is the whitelist's bytes.
//
// Claim: with S the mapped records' indices, ascending, finish gives exactly what
// oem_em_run_cells_records_whitelist_sparse gives on records[S], barcodes[S], names[S], secondary[S], umis[S] under the
// same rules, filters, model and mode, however the input is cut and whichever thread pushes what: order is S[order of the
// one call]; cell_rec_off, group_off, cell_group_off, kept, the discard tables, cell_dups, cell_corrected, the entries'
// offsets and columns, the five status counts and the labels are exact.
//
// A deferred record: the sessions differ.  A deferred record is retained, so it is checked in its batch -- name, UMI,
// ref_id.  If finish rejects it, an error in it has been an error of the session all the same; the one call, which
// decides every barcode before it looks at anything else, never sees that error.
#pragma once

#include <algorithm>
#include <vector>

#include "oem_barcode_table.h"

namespace oem {

constexpr uint8_t kBarcodeExact = 0, kBarcodeCorrected = 1, kBarcodeNoNeighbour = 2, kBarcodeAmbiguous = 3, kBarcodeMissing = 4;
constexpr int kBarcodeStatuses = 5;
constexpr uint8_t kBarcodeDeferred = 5;    // a session's record that waits for the complete counts: never leaves the library
constexpr uint8_t kBarcodeNoPart = 0xff;   // the streamed walk's out_status of an unmapped record (testing only)
constexpr uint32_t kBarcodeNoId = 0xffffffffu;
// in a session's arena: the id of a record that was corrected (the cells' corrected counts come from it at finish); a
// session's whitelist therefore holds at most 2^31 - 1 labels
constexpr uint32_t kBarcodeCorrectedBit = 0x80000000u;
constexpr uint64_t kBarcodeMaxLabel = 64;   // bytes of a label: a wavefront's lanes own a barcode's byte positions
constexpr uint32_t kBarcodeMaxAlphabet = 8; // bytes of an alphabet: it travels as one 8-byte word
constexpr uint64_t kBarcodeNoIndex = ~0ull;

// the chained hash of oem_barcode_table.h before word w0 of the barcode: barcode_hash = barcode_hash_from(prefix, ..., w0)
OEM_HD inline uint64_t barcode_hash_prefix(const uint8_t *p, uint64_t len, uint64_t w0)
{
    uint64_t h = 0x9e3779b97f4a7c15ull ^ len;
    for (uint64_t w = 0; w < w0; ++w) h = barcode_mix(h ^ barcode_word(p, len, w));
    return h;
}
// ... and the rest of it, with `word` in place of the barcode's own word w0
OEM_HD inline uint64_t barcode_hash_from(uint64_t h, const uint8_t *p, uint64_t len, uint64_t w0, uint64_t word)
{
    h = barcode_mix(h ^ word);
    for (uint64_t w = w0 + 1; 8 * w < len; ++w) h = barcode_mix(h ^ barcode_word(p, len, w));
    return barcode_mix(h);
}

// barcode_table_find for the candidate "p[0 .. len) with word w0 replaced by `word`", whose hash the caller has.
OEM_HD inline uint32_t barcode_table_find_candidate(const uint32_t *slot, uint64_t capacity, uint32_t hash_bits, const uint8_t *labels,
                                                    const uint64_t *label_off, const uint8_t *p, uint64_t len, uint64_t w0, uint64_t word,
                                                    uint64_t hash, uint64_t *steps, bool *wrapped)
{
    uint64_t at = barcode_home(hash, hash_bits, capacity);
    for (uint64_t k = 0; k < capacity; ++k) {
        const uint32_t id = slot[at];
        if (id == kBarcodeEmpty) {
            *steps = k + 1;
            return kBarcodeEmpty;
        }
        const uint64_t l0 = label_off[id];
        if (label_off[id + 1] - l0 == len) {
            bool same = true;
            for (uint64_t w = 0; same && 8 * w < len; ++w) same = barcode_word(labels + l0, len, w) == (w == w0 ? word : barcode_word(p, len, w));
            if (same) {
                *steps = k + 1;
                return id;
            }
        }
        if (++at == capacity) {
            at = 0;
            *wrapped = true;
        }
    }
    *steps = capacity;
    return kBarcodeProbeError;
}

// The SMALLEST id among the labels of the table that equal p[0 .. len): equal labels share a home slot and lie in one
// stretch of occupied slots behind it, so the probe goes on to the first free slot.  What proves a whitelist distinct.
OEM_HD inline uint32_t barcode_table_find_smallest(const uint32_t *slot, uint64_t capacity, uint32_t hash_bits, const uint8_t *labels,
                                                   const uint64_t *label_off, const uint8_t *p, uint64_t len)
{
    uint64_t at = barcode_home(barcode_hash(p, len), hash_bits, capacity);
    uint32_t best = kBarcodeEmpty;
    for (uint64_t k = 0; k < capacity; ++k) {
        const uint32_t id = slot[at];
        if (id == kBarcodeEmpty) return best;
        const uint64_t l0 = label_off[id];
        if (id < best && barcode_equal(p, len, labels + l0, label_off[id + 1] - l0)) best = id;
        if (++at == capacity) at = 0;
    }
    return kBarcodeProbeError;
}

// true if one of the bytes of p[0 .. len) is 0
OEM_HD inline bool barcode_has_zero_byte(const uint8_t *p, uint64_t len)
{
    for (uint64_t w = 0; 8 * w < len; ++w) {
        uint64_t v = barcode_word(p, len, w);
        const uint64_t left = len - 8 * w;
        if (left < 8) v |= ~0ull << (8 * left); // the bytes past the end are no bytes of the barcode
        if ((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull) return true;
    }
    return false;
}

// What the candidates of a barcode found: how many neighbours, the largest n among them, how many reach it, and the id of
// one that does (the only one, where that matters).  Votes are merged in any order.
struct BarcodeVote {
    uint32_t found = 0, best_n = 0, n_best = 0, id = kBarcodeNoId;
};
OEM_HD inline void barcode_vote_add(BarcodeVote &v, uint32_t id, uint32_t n)
{
    if (v.found == 0 || n > v.best_n) {
        v.best_n = n;
        v.n_best = 1;
        v.id = id;
    } else if (n == v.best_n) {
        ++v.n_best;
        if (id < v.id) v.id = id;
    }
    ++v.found;
}
OEM_HD inline void barcode_vote_merge(BarcodeVote &a, const BarcodeVote &b)
{
    if (b.found == 0) return;
    if (a.found == 0 || b.best_n > a.best_n) {
        const uint32_t found = a.found + b.found;
        a = b;
        a.found = found;
        return;
    }
    if (b.best_n == a.best_n) {
        a.n_best += b.n_best;
        if (b.id < a.id) a.id = b.id;
    }
    a.found += b.found;
}
// the choice: the status, and *id = the label for kBarcodeCorrected, kBarcodeNoId otherwise
OEM_HD inline uint8_t barcode_vote_decide(const BarcodeVote &v, uint32_t multi, uint32_t *id)
{
    *id = kBarcodeNoId;
    if (v.found == 0) return kBarcodeNoNeighbour;
    if (v.found == 1 || (multi && v.n_best == 1)) {
        *id = v.id;
        return kBarcodeCorrected;
    }
    return kBarcodeAmbiguous;
}

// the choice of a session's batch: what does not depend on the counts is decided, the rest is kBarcodeDeferred
OEM_HD inline uint8_t barcode_vote_decide_or_defer(const BarcodeVote &v, uint32_t multi, uint32_t *id)
{
    if (multi && v.found >= 2) {
        *id = kBarcodeNoId;
        return kBarcodeDeferred;
    }
    return barcode_vote_decide(v, multi, id);
}

// The votes of byte position `pos` of the barcode p[0 .. len), pos < len: every alphabet byte but the barcode's own there
// is tried.  alphabet: its n_alphabet bytes as one word, byte 0 in the low bits.  count: n(w), complete.
OEM_HD inline void barcode_vote_position(BarcodeVote &v, const uint32_t *slot, uint64_t capacity, uint32_t hash_bits, const uint8_t *labels,
                                         const uint64_t *label_off, const uint32_t *count, uint64_t alphabet, uint32_t n_alphabet,
                                         const uint8_t *p, uint64_t len, uint64_t pos, uint64_t *longest, bool *wrapped, bool *broken)
{
    const uint64_t w0 = pos / 8, sh = 8 * (pos % 8);
    const uint64_t own = barcode_word(p, len, w0), prefix = barcode_hash_prefix(p, len, w0);
    for (uint32_t a = 0; a < n_alphabet; ++a) {
        const uint64_t byte = (alphabet >> (8 * a)) & 0xffull;
        if (byte == ((own >> sh) & 0xffull)) continue;
        const uint64_t word = (own & ~(0xffull << sh)) | (byte << sh);
        uint64_t steps = 0;
        const uint32_t id = barcode_table_find_candidate(slot, capacity, hash_bits, labels, label_off, p, len, w0, word,
                                                         barcode_hash_from(prefix, p, len, w0, word), &steps, wrapped);
        if (steps > *longest) *longest = steps;
        if (id == kBarcodeProbeError) *broken = true;
        else if (id != kBarcodeEmpty) barcode_vote_add(v, id, count[id]);
    }
}

// the bit of a label length (1 .. 64) in the mask of the whitelist's lengths
OEM_HD inline uint64_t barcode_len_bit(uint64_t len) { return len >= 1 && len <= kBarcodeMaxLabel ? 1ull << (len - 1) : 0ull; }

// What the host walk reports besides its outputs.
struct BarcodeCorrectHost {
    // the first device-found error in the order of the call: a label with a 0 byte; two equal labels (i < j, the pair that
    // is smallest with i first, i being the smallest index of j's bytes); a barcode with a 0 byte (the smallest record)
    uint64_t zero_label = kBarcodeNoIndex, equal_i = kBarcodeNoIndex, equal_j = kBarcodeNoIndex, zero_barcode = kBarcodeNoIndex;
    uint64_t longest_probe = 0;
    bool wrapped = false, broken = false;
    bool bad() const { return zero_label != kBarcodeNoIndex || equal_j != kBarcodeNoIndex || zero_barcode != kBarcodeNoIndex || broken; }
};

// The whitelist of a host walk: the labels checked, the table over them, the lengths' mask and the alphabet as a word.
struct BarcodeWhitelistHost {
    BarcodeTableHost t;
    uint64_t len_mask = 0, alpha = 0;
    BarcodeWhitelistHost(uint64_t slots0, uint32_t hash_bits) : t(slots0, hash_bits) {}
};
// Fills wl and info's label errors and table words; with info->bad() nothing may be looked up.
inline void barcode_whitelist_host(const uint8_t *labels, const uint64_t *label_off, uint32_t n_labels, const uint8_t *alphabet,
                                   uint32_t n_alphabet, BarcodeWhitelistHost *wl, BarcodeCorrectHost *info)
{
    const uint64_t W = n_labels;
    BarcodeTableHost &t = wl->t;
    for (uint32_t a = 0; a < n_alphabet; ++a) wl->alpha |= (uint64_t)alphabet[a] << (8 * a);
    for (uint64_t w = 0; w < W; ++w) {
        const uint64_t l0 = label_off[w], len = label_off[w + 1] - l0;
        if (barcode_has_zero_byte(labels + l0, len)) {
            info->zero_label = w;
            return;
        }
        wl->len_mask |= barcode_len_bit(len);
    }
    // the table: every label goes in, then a lookup of every label proves it distinct
    t.labels.assign(labels, labels + label_off[W]);
    t.label_off.assign(label_off, label_off + W + 1);
    t.add_from(0);
    for (uint64_t j = 0; j < W && !t.broken; ++j) {
        const uint64_t l0 = label_off[j];
        const uint32_t i = barcode_table_find_smallest(t.slot.data(), t.slot.size(), t.hash_bits, labels, label_off, labels + l0, label_off[j + 1] - l0);
        if (i == kBarcodeProbeError || i == kBarcodeEmpty) t.broken = true;
        else if (i != j && (info->equal_j == kBarcodeNoIndex || i < info->equal_i)) {
            info->equal_i = i;
            info->equal_j = j;
        }
    }
    info->longest_probe = t.longest_probe;
    info->wrapped = t.wrapped;
    info->broken = t.broken;
}
// the vote of the miss p[0 .. len) with the counts as they stand
inline BarcodeVote barcode_vote_host(const BarcodeWhitelistHost &wl, const uint32_t *count, uint32_t n_alphabet, const uint8_t *p, uint64_t len,
                                     BarcodeCorrectHost *info)
{
    const BarcodeTableHost &t = wl.t;
    BarcodeVote v;
    for (uint64_t pos = 0; pos < len; ++pos) {
        BarcodeVote at;
        barcode_vote_position(at, t.slot.data(), t.slot.size(), t.hash_bits, t.labels.data(), t.label_off.data(), count, wl.alpha, n_alphabet, p,
                              len, pos, &info->longest_probe, &info->wrapped, &info->broken);
        barcode_vote_merge(v, at);
    }
    return v;
}
// The exact pass of one record: kBarcodeMissing, kBarcodeNoNeighbour (a length no label has), kBarcodeExact with *id and
// n(w) raised, or kBarcodeDeferred for a miss that the neighbour pass decides.  *zero: the barcode holds a 0 byte.
inline uint8_t barcode_exact_host(BarcodeWhitelistHost &wl, uint32_t *count, const uint8_t *p, uint64_t len, uint32_t *id, bool *zero)
{
    *id = kBarcodeNoId;
    *zero = false;
    if (len == 0) return kBarcodeMissing;
    if (barcode_has_zero_byte(p, len)) {
        *zero = true;
        return kBarcodeMissing;
    }
    if (!(wl.len_mask & barcode_len_bit(len))) return kBarcodeNoNeighbour; // no label has this length
    const uint32_t w = wl.t.find(p, len);
    if (w == kBarcodeEmpty) return kBarcodeDeferred;
    if (w == kBarcodeProbeError) return kBarcodeNoNeighbour; // (t.broken is set)
    *id = w;
    ++count[w];
    return kBarcodeExact;
}
// The cells of the ids (kBarcodeNoId: in no cell): numbered by their first accepted record, input order inside.
inline void barcode_cells_host(const std::vector<uint32_t> &id, uint64_t W, std::vector<uint64_t> *order, std::vector<uint64_t> *cro,
                               std::vector<uint32_t> *cell_label)
{
    std::vector<uint32_t> cell_of(W, kBarcodeNoId);
    std::vector<uint64_t> size;
    cell_label->clear();
    for (uint64_t i = 0; i < id.size(); ++i) {
        if (id[i] == kBarcodeNoId) continue;
        if (cell_of[id[i]] == kBarcodeNoId) {
            cell_of[id[i]] = (uint32_t)size.size();
            size.push_back(0);
            cell_label->push_back(id[i]);
        }
        ++size[cell_of[id[i]]];
    }
    cro->assign(size.size() + 1, 0);
    for (size_t c = 0; c < size.size(); ++c) (*cro)[c + 1] = (*cro)[c] + size[c];
    order->assign(cro->back(), 0);
    std::vector<uint64_t> at(cro->begin(), cro->end() - 1);
    for (uint64_t i = 0; i < id.size(); ++i)
        if (id[i] != kBarcodeNoId) (*order)[at[cell_of[id[i]]]++] = i;
}

// The host walk.  The arguments are checked (oem_correct_barcodes' checks before device use).  Each output or NULL:
// out_id / out_status (n_records), out_order (capacity n_records), out_cell_rec_off (capacity n_records + 1), out_counts
// (kBarcodeStatuses).  With info.bad() the outputs are unspecified.  hash_bits / slots0: the table's (testing: short
// hashes make the probes long and wrap).
inline BarcodeCorrectHost correct_barcodes_host(const uint8_t *labels, const uint64_t *label_off, uint32_t n_labels, uint32_t multi,
                                                const uint8_t *alphabet, uint32_t n_alphabet, const uint8_t *barcodes,
                                                const uint64_t *barcode_off, uint64_t n_records, uint32_t *out_id, uint8_t *out_status,
                                                uint32_t *out_order, uint64_t *out_cell_rec_off, uint64_t *out_n_cells,
                                                uint64_t *out_n_accepted, uint64_t *out_counts, uint32_t hash_bits = 64,
                                                uint64_t slots0 = kBarcodeTableSlots0)
{
    BarcodeCorrectHost info;
    *out_n_cells = 0;
    *out_n_accepted = 0;
    const uint64_t W = n_labels, n = n_records;
    BarcodeWhitelistHost wl(slots0, hash_bits);
    barcode_whitelist_host(labels, label_off, n_labels, alphabet, n_alphabet, &wl, &info);
    if (info.bad()) return info;

    // the exact pass: ids, statuses and n(w)
    std::vector<uint32_t> id(n, kBarcodeNoId), count(W, 0);
    std::vector<uint8_t> status(n, kBarcodeMissing);
    std::vector<uint64_t> misses;
    for (uint64_t i = 0; i < n; ++i) {
        bool zero = false;
        status[i] = barcode_exact_host(wl, count.data(), barcodes + barcode_off[i], barcode_off[i + 1] - barcode_off[i], &id[i], &zero);
        if (zero) {
            info.zero_barcode = i;
            return info;
        }
        if (status[i] == kBarcodeDeferred) misses.push_back(i);
    }
    info.longest_probe = wl.t.longest_probe;
    info.wrapped = wl.t.wrapped;
    info.broken = wl.t.broken;
    // the neighbour pass, over the misses only and with the counts complete
    for (const uint64_t i : misses) {
        const uint64_t b0 = barcode_off[i];
        status[i] = barcode_vote_decide(barcode_vote_host(wl, count.data(), n_alphabet, barcodes + b0, barcode_off[i + 1] - b0, &info), multi, &id[i]);
    }
    if (info.broken) return info;

    // the cells: numbered by their first accepted record, input order inside
    std::vector<uint64_t> order, cro;
    std::vector<uint32_t> cell_label;
    barcode_cells_host(id, W, &order, &cro, &cell_label);
    uint64_t counts[kBarcodeStatuses] = {0, 0, 0, 0, 0};
    for (uint64_t i = 0; i < n; ++i) ++counts[status[i]];
    if (out_order)
        for (size_t k = 0; k < order.size(); ++k) out_order[k] = (uint32_t)order[k];
    if (out_cell_rec_off) std::copy(cro.begin(), cro.end(), out_cell_rec_off);
    if (out_id) std::copy(id.begin(), id.end(), out_id);
    if (out_status) std::copy(status.begin(), status.end(), out_status);
    if (out_counts) std::copy(counts, counts + kBarcodeStatuses, out_counts);
    *out_n_cells = cro.size() - 1;
    *out_n_accepted = order.size();
    return info;
}

// The streamed walk ("The rule in a session"): the records [batch_off[b], batch_off[b + 1]) are batch b, n_batches >= 0
// batches from 0; unmapped (or NULL: none): a flag per record.  The walk does what the session does, in its order: per
// batch the exact pass and the neighbour pass that decides or defers, the rejected records dropped, the retained ones
// kept with an id and the deferred ones' positions pending; at the end the pending pass with the complete counts and the
// cells from the ids.  Outputs as correct_barcodes_host's, indexed by the record's index in the whole input, out_order
// 64 bits wide; an unmapped record has kBarcodeNoId / kBarcodeNoPart and is in no count.  out_cell_label (capacity
// n_labels): the cells' labels; out_cell_corrected (likewise): the records of every cell that were corrected;
// *out_n_rejected: the mapped records dropped, per batch or at the end; *out_n_deferred: the records that waited.
// zero_barcode names a MAPPED record; an unmapped record's barcode is never examined.
inline BarcodeCorrectHost correct_barcodes_stream_host(const uint8_t *labels, const uint64_t *label_off, uint32_t n_labels, uint32_t multi,
                                                       const uint8_t *alphabet, uint32_t n_alphabet, const uint8_t *barcodes,
                                                       const uint64_t *barcode_off, const uint64_t *batch_off, uint64_t n_batches,
                                                       const uint8_t *unmapped, uint32_t *out_id, uint8_t *out_status, uint64_t *out_order,
                                                       uint64_t *out_cell_rec_off, uint32_t *out_cell_label, uint64_t *out_cell_corrected,
                                                       uint64_t *out_n_cells, uint64_t *out_n_accepted, uint64_t *out_counts,
                                                       uint64_t *out_n_rejected, uint64_t *out_n_deferred, uint32_t hash_bits = 64,
                                                       uint64_t slots0 = kBarcodeTableSlots0)
{
    BarcodeCorrectHost info;
    *out_n_cells = 0;
    *out_n_accepted = 0;
    *out_n_rejected = 0;
    *out_n_deferred = 0;
    const uint64_t W = n_labels, n = n_batches ? batch_off[n_batches] : 0;
    BarcodeWhitelistHost wl(slots0, hash_bits); // the session's: built once, when the rule is set
    barcode_whitelist_host(labels, label_off, n_labels, alphabet, n_alphabet, &wl, &info);
    if (info.bad()) return info;
    std::vector<uint32_t> count(W, 0);                  // the session's n(w): never reset
    std::vector<uint64_t> arena_rec;                    // the arena: the retained records' input indices ...
    std::vector<uint32_t> arena_id;                     // ... and their ids (kBarcodeCorrectedBit: corrected)
    std::vector<uint64_t> pending;                      // arena positions of the deferred records
    std::vector<uint8_t> status(n, kBarcodeNoPart);
    uint64_t counts[kBarcodeStatuses] = {0, 0, 0, 0, 0};
    for (uint64_t b = 0; b < n_batches; ++b) {
        // the exact pass over the batch's mapped records
        std::vector<uint64_t> mapped, misses;
        std::vector<uint32_t> id;
        for (uint64_t i = batch_off[b]; i < batch_off[b + 1]; ++i) {
            if (unmapped && unmapped[i]) continue;
            bool zero = false;
            uint32_t w = kBarcodeNoId;
            status[i] = barcode_exact_host(wl, count.data(), barcodes + barcode_off[i], barcode_off[i + 1] - barcode_off[i], &w, &zero);
            if (zero) {
                info.zero_barcode = i;
                return info;
            }
            if (status[i] == kBarcodeDeferred) misses.push_back(mapped.size());
            mapped.push_back(i);
            id.push_back(w);
        }
        info.longest_probe = std::max(info.longest_probe, wl.t.longest_probe);
        info.wrapped = info.wrapped || wl.t.wrapped;
        info.broken = info.broken || wl.t.broken;
        // the neighbour pass with the counts as they stand: decided, or deferred
        for (const uint64_t k : misses) {
            const uint64_t i = mapped[k], b0 = barcode_off[i];
            const BarcodeVote v = barcode_vote_host(wl, count.data(), n_alphabet, barcodes + b0, barcode_off[i + 1] - b0, &info);
            status[i] = barcode_vote_decide_or_defer(v, multi, &id[k]);
            if (status[i] == kBarcodeCorrected) id[k] |= kBarcodeCorrectedBit;
        }
        if (info.broken) return info;
        // the retained records enter the arena; the rest is dropped here
        for (uint64_t k = 0; k < mapped.size(); ++k) {
            const uint8_t st = status[mapped[k]];
            if (st == kBarcodeDeferred) {
                pending.push_back(arena_rec.size());
                ++*out_n_deferred;
            } else {
                ++counts[st];
                if (st > kBarcodeCorrected) {
                    ++*out_n_rejected;
                    continue;
                }
            }
            arena_rec.push_back(mapped[k]);
            arena_id.push_back(id[k]);
        }
    }
    // finish: the pending records with the complete counts
    for (const uint64_t pos : pending) {
        const uint64_t i = arena_rec[pos], b0 = barcode_off[i];
        const BarcodeVote v = barcode_vote_host(wl, count.data(), n_alphabet, barcodes + b0, barcode_off[i + 1] - b0, &info);
        status[i] = barcode_vote_decide(v, multi, &arena_id[pos]);
        ++counts[status[i]];
        if (status[i] == kBarcodeCorrected) arena_id[pos] |= kBarcodeCorrectedBit;
        else ++*out_n_rejected;
    }
    if (info.broken) return info;
    // the cells from the arena's ids
    std::vector<uint32_t> key(arena_id.size());
    for (size_t p = 0; p < key.size(); ++p) key[p] = arena_id[p] == kBarcodeNoId ? kBarcodeNoId : arena_id[p] & ~kBarcodeCorrectedBit;
    std::vector<uint64_t> order, cro;
    std::vector<uint32_t> cell_label;
    barcode_cells_host(key, W, &order, &cro, &cell_label);
    const uint64_t nc = cro.size() - 1;
    if (out_order)
        for (size_t k = 0; k < order.size(); ++k) out_order[k] = arena_rec[order[k]];
    if (out_cell_rec_off) std::copy(cro.begin(), cro.end(), out_cell_rec_off);
    if (out_cell_label) std::copy(cell_label.begin(), cell_label.end(), out_cell_label);
    if (out_cell_corrected)
        for (uint64_t c = 0; c < nc; ++c) {
            out_cell_corrected[c] = 0;
            for (uint64_t k = cro[c]; k < cro[c + 1]; ++k) out_cell_corrected[c] += (arena_id[order[k]] & kBarcodeCorrectedBit) != 0;
        }
    if (out_id) {
        std::fill(out_id, out_id + n, kBarcodeNoId);
        for (size_t p = 0; p < key.size(); ++p) out_id[arena_rec[p]] = key[p];
    }
    if (out_status) std::copy(status.begin(), status.end(), out_status);
    if (out_counts) std::copy(counts, counts + kBarcodeStatuses, out_counts);
    *out_n_cells = nc;
    *out_n_accepted = order.size();
    return info;
}

// The argument checks of a barcode rule before any device use, as a message (NULL: the rule is good).  The public header
// is not included here, so the rule arrives as its fields.
inline const char *barcode_rule_problem(const uint8_t *labels, const uint64_t *label_off, uint32_t n_labels, uint32_t multi,
                                        const uint8_t *alphabet, uint32_t n_alphabet, uint64_t *which)
{
    *which = 0;
    if (!labels || !label_off) return "rule->labels or rule->label_off is NULL";
    if (n_labels == 0) return "rule->n_labels is 0: a whitelist holds a label at least";
    if (label_off[0] != 0) return "rule->label_off must start at 0";
    for (uint32_t w = 0; w < n_labels; ++w) {
        *which = w;
        if (label_off[w + 1] < label_off[w]) return "rule->label_off must be non-decreasing (label %llu)";
        if (label_off[w + 1] == label_off[w]) return "label %llu of the whitelist is empty";
        if (label_off[w + 1] - label_off[w] > kBarcodeMaxLabel) return "label %llu of the whitelist has more than 64 bytes";
    }
    *which = multi;
    if (multi > 1) return "rule->multi = %llu is neither 0 nor 1";
    if (alphabet) {
        *which = n_alphabet;
        if (n_alphabet == 0) return "rule->alphabet is given and rule->n_alphabet is 0";
        if (n_alphabet > kBarcodeMaxAlphabet) return "rule->n_alphabet = %llu: an alphabet has at most 8 bytes";
        for (uint32_t a = 0; a < n_alphabet; ++a) {
            *which = a;
            if (alphabet[a] == 0) return "byte %llu of rule->alphabet is 0";
            for (uint32_t b = 0; b < a; ++b)
                if (alphabet[a] == alphabet[b]) return "byte %llu of rule->alphabet repeats an earlier one";
        }
    }
    return nullptr;
}

} // namespace oem
