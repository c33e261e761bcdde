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
#pragma once

#include <vector>

#include "oem_barcode_table.h"

namespace oem {

constexpr uint8_t kBarcodeExact = 0, kBarcodeCorrected = 1, kBarcodeNoNeighbour = 2, kBarcodeAmbiguous = 3, kBarcodeMissing = 4;
constexpr int kBarcodeStatuses = 5;
constexpr uint32_t kBarcodeNoId = 0xffffffffu;
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
    uint64_t len_mask = 0, alpha = 0;
    for (uint32_t a = 0; a < n_alphabet; ++a) alpha |= (uint64_t)alphabet[a] << (8 * a);
    for (uint64_t w = 0; w < W; ++w) {
        const uint64_t l0 = label_off[w], len = label_off[w + 1] - l0;
        if (barcode_has_zero_byte(labels + l0, len)) {
            info.zero_label = w;
            return info;
        }
        len_mask |= barcode_len_bit(len);
    }
    // the table: every label goes in, then a lookup of every label proves it distinct
    BarcodeTableHost t(slots0, hash_bits);
    t.labels.assign(labels, labels + label_off[W]);
    t.label_off.assign(label_off, label_off + W + 1);
    t.add_from(0);
    for (uint64_t j = 0; j < W && !t.broken; ++j) {
        const uint64_t l0 = label_off[j];
        const uint32_t i = barcode_table_find_smallest(t.slot.data(), t.slot.size(), hash_bits, labels, label_off, labels + l0, label_off[j + 1] - l0);
        if (i == kBarcodeProbeError || i == kBarcodeEmpty) t.broken = true;
        else if (i != j && (info.equal_j == kBarcodeNoIndex || i < info.equal_i)) {
            info.equal_i = i;
            info.equal_j = j;
        }
    }
    info.longest_probe = t.longest_probe;
    info.wrapped = t.wrapped;
    info.broken = t.broken;
    if (info.bad()) return info;

    // the exact pass: ids, statuses and n(w)
    std::vector<uint32_t> id(n, kBarcodeNoId), count(W, 0);
    std::vector<uint8_t> status(n, kBarcodeMissing);
    std::vector<uint64_t> misses;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t b0 = barcode_off[i], len = barcode_off[i + 1] - b0;
        if (len == 0) continue;
        if (barcode_has_zero_byte(barcodes + b0, len)) {
            info.zero_barcode = i;
            return info;
        }
        status[i] = kBarcodeNoNeighbour;
        if (!(len_mask & barcode_len_bit(len))) continue; // no label has this length
        const uint32_t w = t.find(barcodes + b0, len);
        if (w == kBarcodeEmpty) {
            misses.push_back(i);
        } else if (w != kBarcodeProbeError) {
            id[i] = w;
            status[i] = kBarcodeExact;
            ++count[w];
        }
    }
    // the neighbour pass, over the misses only and with the counts complete
    bool wrapped = t.wrapped, broken = t.broken;
    uint64_t longest = t.longest_probe;
    for (const uint64_t i : misses) {
        const uint64_t b0 = barcode_off[i], len = barcode_off[i + 1] - b0;
        BarcodeVote v;
        for (uint64_t pos = 0; pos < len; ++pos) {
            BarcodeVote at;
            barcode_vote_position(at, t.slot.data(), t.slot.size(), hash_bits, labels, label_off, count.data(), alpha, n_alphabet,
                                  barcodes + b0, len, pos, &longest, &wrapped, &broken);
            barcode_vote_merge(v, at);
        }
        status[i] = barcode_vote_decide(v, multi, &id[i]);
    }
    info.longest_probe = longest;
    info.wrapped = wrapped;
    info.broken = broken;
    if (broken) return info;

    // the cells: numbered by their first accepted record, input order inside
    std::vector<uint32_t> cell_of(W, kBarcodeNoId);
    std::vector<uint64_t> size;
    uint64_t counts[kBarcodeStatuses] = {0, 0, 0, 0, 0}, n_accepted = 0;
    for (uint64_t i = 0; i < n; ++i) {
        ++counts[status[i]];
        if (id[i] == kBarcodeNoId) continue;
        if (cell_of[id[i]] == kBarcodeNoId) {
            cell_of[id[i]] = (uint32_t)size.size();
            size.push_back(0);
        }
        ++size[cell_of[id[i]]];
        ++n_accepted;
    }
    std::vector<uint64_t> cro(size.size() + 1, 0);
    for (size_t c = 0; c < size.size(); ++c) cro[c + 1] = cro[c] + size[c];
    if (out_order) {
        std::vector<uint64_t> at(cro.begin(), cro.end() - 1);
        for (uint64_t i = 0; i < n; ++i)
            if (id[i] != kBarcodeNoId) out_order[at[cell_of[id[i]]]++] = (uint32_t)i;
    }
    if (out_cell_rec_off) std::copy(cro.begin(), cro.end(), out_cell_rec_off);
    if (out_id) std::copy(id.begin(), id.end(), out_id);
    if (out_status) std::copy(status.begin(), status.end(), out_status);
    if (out_counts) std::copy(counts, counts + kBarcodeStatuses, out_counts);
    *out_n_cells = size.size();
    *out_n_accepted = n_accepted;
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
