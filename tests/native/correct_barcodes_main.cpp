// Stand-alone host program over the barcode rule of oarfish_amd/csrc/oem_barcode_correct.h (tests/test_correct_barcodes.py
// builds it with the address and undefined-behaviour sanitizers).  Cases on stdin, one answer line each:
//   R n_labels n_records multi alphabet_as_hex hash_bits slots0
//   then n_labels lines   label_as_hex
//   then n_records lines  barcode_as_hex          ("-" for an empty barcode)
//       -> ok | id | status | order | cell_rec_off | counts
//       or rule message        (the rule's argument checks)
//       or zerolabel w         (a label with a 0 byte)
//       or equal i j           (two equal labels)
//       or zerobarcode i       (a barcode with a 0 byte)
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

template <typename V>
static void put(const V &v, size_t n)
{
    printf(" |");
    for (size_t i = 0; i < n; ++i) printf(" %" PRIu64, (uint64_t)v[i]);
}

int main()
{
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] != 'R') return 2;
        uint64_t W, n, slots0;
        uint32_t multi, hash_bits;
        char hex[1024];
        if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu32 " %1023s %" SCNu32 " %" SCNu64, &W, &n, &multi, hex, &hash_bits, &slots0) != 6) return 2;
        // exactly the bytes of the strings and exactly the entries of every array: one read past them is a sanitizer report
        std::vector<uint8_t> alphabet, labels, blob;
        unhex(hex, &alphabet);
        std::vector<uint64_t> label_off(W + 1, 0), off(n + 1, 0);
        for (uint64_t w = 0; w < W; ++w) {
            if (scanf("%1023s", hex) != 1) return 2;
            unhex(hex, &labels);
            label_off[w + 1] = labels.size();
        }
        for (uint64_t i = 0; i < n; ++i) {
            if (scanf("%1023s", hex) != 1) return 2;
            unhex(hex, &blob);
            off[i + 1] = blob.size();
        }
        uint64_t which = 0;
        const char *problem = oem::barcode_rule_problem(labels.data(), label_off.data(), (uint32_t)W, multi, alphabet.data(),
                                                        (uint32_t)alphabet.size(), &which);
        if (problem) {
            printf("rule ");
            printf(problem, (unsigned long long)which);
            putchar('\n');
            continue;
        }
        std::vector<uint32_t> id(n), order(n);
        std::vector<uint8_t> status(n);
        std::vector<uint64_t> cro(n + 1), counts(oem::kBarcodeStatuses);
        uint64_t n_cells = 0, n_accepted = 0;
        const oem::BarcodeCorrectHost info =
            oem::correct_barcodes_host(labels.data(), label_off.data(), (uint32_t)W, multi, alphabet.data(), (uint32_t)alphabet.size(), blob.data(),
                                       off.data(), n, id.data(), status.data(), order.data(), cro.data(), &n_cells, &n_accepted, counts.data(),
                                       hash_bits, slots0);
        if (info.zero_label != oem::kBarcodeNoIndex) {
            printf("zerolabel %" PRIu64 "\n", info.zero_label);
        } else if (info.broken) {
            printf("broken\n");
        } else if (info.equal_j != oem::kBarcodeNoIndex) {
            printf("equal %" PRIu64 " %" PRIu64 "\n", info.equal_i, info.equal_j);
        } else if (info.zero_barcode != oem::kBarcodeNoIndex) {
            printf("zerobarcode %" PRIu64 "\n", info.zero_barcode);
        } else {
            printf("ok");
            put(id, n);
            put(status, n);
            put(order, n_accepted);
            put(cro, n_cells + 1);
            put(counts, counts.size());
            putchar('\n');
        }
    }
    return 0;
}
