// Stand-alone host program over the streamed barcode rule of oarfish_amd/csrc/oem_barcode_correct.h ("The rule in a
// session"; tests/test_correct_barcodes_stream.py builds it with the address and undefined-behaviour sanitizers).  Cases on
// stdin, one answer line each:
//   S n_labels n_records multi pairs hash_bits slots0
//   then n_labels lines   label_as_hex
//   then n_records lines  barcode_as_hex unmapped          ("-" for an empty barcode)
//       -> ok cuttings accepted cells rejected deferred
//       or differ cut_a cut_b what
// The program itself holds correct_barcodes_stream_host at every single cut (pairs = 1: and at every pair of cuts) to
// correct_barcodes_host on the mapped records' arrays, which it gathers here.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../oarfish_amd/csrc/oem_barcode_correct.h"

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

static void unhex(const char *hex, std::vector<uint8_t> *blob)
{
    if (hex[0] == '-') return;
    for (size_t k = 0; hex[k] && hex[k + 1]; k += 2) blob->push_back((uint8_t)(hexval(hex[k]) * 16 + hexval(hex[k + 1])));
}

int main()
{
    static const uint8_t acgt[4] = {'A', 'C', 'G', 'T'};
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] != 'S') return 2;
        uint64_t W, n, slots0;
        uint32_t multi, pairs, hash_bits;
        char hex[1024];
        if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64, &W, &n, &multi, &pairs, &hash_bits, &slots0) != 6) return 2;
        // exactly the bytes of the strings and exactly the entries of every array: one read past them is a sanitizer report
        std::vector<uint8_t> labels, blob, sub_blob, unmapped(n, 0);
        std::vector<uint64_t> label_off(W + 1, 0), off(n + 1, 0), sub_off(1, 0), S;
        for (uint64_t w = 0; w < W; ++w) {
            if (scanf("%1023s", hex) != 1) return 2;
            unhex(hex, &labels);
            label_off[w + 1] = labels.size();
        }
        for (uint64_t i = 0; i < n; ++i) {
            unsigned um = 0;
            if (scanf("%1023s %u", hex, &um) != 2) return 2;
            unhex(hex, &blob);
            off[i + 1] = blob.size();
            unmapped[i] = (uint8_t)um;
            if (!um) {
                unhex(hex, &sub_blob);
                sub_off.push_back(sub_blob.size());
                S.push_back(i);
            }
        }
        // the one-shot walk on the mapped records
        const uint64_t m = S.size();
        std::vector<uint32_t> id1(m), order1(m);
        std::vector<uint8_t> st1(m);
        std::vector<uint64_t> cro1(m + 1), counts1(oem::kBarcodeStatuses);
        uint64_t nc1 = 0, na1 = 0;
        const oem::BarcodeCorrectHost one =
            oem::correct_barcodes_host(labels.data(), label_off.data(), (uint32_t)W, multi, acgt, 4, sub_blob.data(), sub_off.data(), m, id1.data(),
                                       st1.data(), order1.data(), cro1.data(), &nc1, &na1, counts1.data(), hash_bits, slots0);
        if (one.bad()) return 3;
        // the streamed walk at every cutting
        uint64_t cuttings = 0, rejected = 0, deferred = 0;
        bool same = true;
        for (uint64_t a = 0; a <= n && same; ++a)
            for (uint64_t b = pairs ? a : n; b <= n && same; ++b) {
                const uint64_t batch_off[4] = {0, a, b, n};
                std::vector<uint32_t> id(n), cell_label(W);
                std::vector<uint8_t> st(n);
                std::vector<uint64_t> order(n), cro(n + 1), cell_corr(W), counts(oem::kBarcodeStatuses);
                uint64_t nc = 0, na = 0;
                const oem::BarcodeCorrectHost got = oem::correct_barcodes_stream_host(
                    labels.data(), label_off.data(), (uint32_t)W, multi, acgt, 4, blob.data(), off.data(), batch_off, 3, unmapped.data(), id.data(),
                    st.data(), order.data(), cro.data(), cell_label.data(), cell_corr.data(), &nc, &na, counts.data(), &rejected, &deferred, hash_bits,
                    slots0);
                ++cuttings;
                const char *what = nullptr;
                if (got.bad()) what = "bad";
                else if (nc != nc1 || na != na1) what = "dims";
                else if (counts != counts1) what = "counts";
                for (uint64_t k = 0; k < m && !what; ++k)
                    if (id[S[k]] != id1[k] || st[S[k]] != st1[k]) what = "id or status";
                for (uint64_t i = 0; i < n && !what; ++i)
                    if (unmapped[i] && (id[i] != oem::kBarcodeNoId || st[i] != oem::kBarcodeNoPart)) what = "an unmapped record";
                for (uint64_t k = 0; k < na1 && !what; ++k)
                    if (order[k] != S[order1[k]]) what = "order";
                for (uint64_t c = 0; c <= nc1 && !what; ++c)
                    if (cro[c] != cro1[c]) what = "cell_rec_off";
                for (uint64_t c = 0; c < nc1 && !what; ++c) {
                    uint64_t corr = 0;
                    for (uint64_t k = cro1[c]; k < cro1[c + 1]; ++k) corr += st1[order1[k]] == oem::kBarcodeCorrected;
                    if (cell_label[c] != id1[order1[cro1[c]]] || cell_corr[c] != corr) what = "the cells' labels or corrected counts";
                }
                if (what) {
                    printf("differ %" PRIu64 " %" PRIu64 " %s\n", a, b, what);
                    same = false;
                }
            }
        if (same) printf("ok %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", cuttings, na1, nc1, rejected, deferred);
    }
    return 0;
}
